"""Per-phase timeline of the persistent Winograd boundary kernel (round 6): build a library with the trace hooks and run this against it.
    tools/experiments/mk_variant.sh trace wino63_kernels.hip -DW63_TRACE=1
    gpurun -- 'MYOLO_LIB=tools/_ab/lib_trace.so python tools/experiments/w63/trace_persistent.py'
Every wave of the first 256 workgroups stamps s_memtime at the top of iterations 8..11, after its first pass (the wait for the prefetched rows), before the barrier,
after it and after its stores were issued (csrc/wino63_kernels.hip: W63_T).  trace_persistent_none.py: the same for the output transform (no back half);
trace_one_unit.py: the one-unit kernels of rounds 3-5 (residency per CU from HW_ID, phases per wave)."""
import os, sys, ctypes, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import torch
from myolo import _ext as X
dev = "cuda:0"
NR, C = 4704, 256
pe = X.wino63_plane_elems(NR, C)
Mp, Vn, b, sc, sh = torch.randn(pe, device=dev), torch.empty(pe, device=dev), torch.randn(C, device=dev), torch.randn(C, device=dev), torch.randn(C, device=dev)
st = X.stream()
for _ in range(3):
    X.call("myolo_wino63_boundary", X.ptr(Mp), X.ptr(b), X.ptr(sc), X.ptr(sh), 1, None, None, 0, None, 0, X.ptr(Vn), NR, C, st)
torch.cuda.synchronize()
lib = ctypes.CDLL(os.environ["MYOLO_LIB"])
n = 8192 * 9 * 8
buf = np.zeros(n, np.uint64)
assert lib.myolo_w63_trace_read(ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(n * 8)) == 0
t = buf[:256 * 4 * 9 * 8].reshape(256, 4, 9, 8).astype(np.int64)
names = ["top->first pass done (waits for the loads)", "->front done", "->barrier passed", "->back + stores issued"]
d = t[..., 1:5] - t[..., 0:4]
for w in range(9):
    print("wave %d: " % w + "  ".join("%s %.0f" % (names[k], d[:, :, w, k].mean()) for k in range(4)))
it = t[:, 1:, :, 0] - t[:, :-1, :, 0]
print("cycles per unit (top to top): mean %.0f  p10 %.0f p90 %.0f" % (it.mean(), np.percentile(it, 10), np.percentile(it, 90)))
