#!/usr/bin/env python
"""What a pass of the anchor k-means costs (profiles/anchors_notes.md records a run), one JSON line.  n = 1 000 000 seeded synthetic sizes in
1 .. 224, k = 9, 8 restarts in one call of myolo_anchor_kmeans:
  device  milliseconds per pass (one assignment launch over all 8 runs + the update launch), from the difference of two calls with max_iter = LONG
          (lowered to below the passes of the run that stops first) and max_iter = SHORT -- the set-up and the final mean-IoU pass are in both and cancel, the host's reads of the runs' flags (one every four
          passes) stay in: they are part of what a pass costs; REPS repetitions, the median and every repetition reported;
  host    the same passes of a vectorised numpy float64 restatement, the (run, half of the points) pairs spread over 16 threads (numpy releases
          the GIL in its loops), HOST_PASSES passes timed.
Before anything is timed the device's centroids after HOST_PASSES passes are compared with the host's, bit for bit.  The one condition checked:
the device is not slower than the host restatement at this size.
  python tools/anchors_rate.py [N=1000000] [SHORT=4] [LONG=132] [REPS=5] [HOST_PASSES=2]
"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

over = dict(a.split("=", 1) for a in sys.argv[1:])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo import _ext as X                                    # noqa: E402
from myolo.anchors import KMAX, initial_centroids              # noqa: E402

N, SHORT, LONG = int(over.get("N", 1000000)), int(over.get("SHORT", 4)), int(over.get("LONG", 132))
REPS, HOST_PASSES = int(over.get("REPS", 5)), int(over.get("HOST_PASSES", 2))
K, RUNS, THREADS, CHUNK = 9, 8, 16, 1 << 16
assert torch.cuda.is_available(), "anchors_rate needs a GPU: a rate measured anywhere else says nothing"
dev = torch.device("cuda:0")
wh = np.random.RandomState(0).randint(1, 225, (N, 2)).astype(np.int32)
starts = initial_centroids(wh, K, RUNS, 0)

# ---- device
wh_d = torch.from_numpy(wh).to(dev)
run_k = np.full(RUNS, K, np.int32)
counts = torch.empty((RUNS, KMAX), dtype=torch.int64, device=dev)
iters, conv = torch.empty(RUNS, dtype=torch.int32, device=dev), torch.empty(RUNS, dtype=torch.int32, device=dev)
miou = torch.empty(RUNS, dtype=torch.float64, device=dev)
ws = torch.empty(X.anchor_kmeans_ws_bytes(N, RUNS), dtype=torch.uint8, device=dev)
pad = np.zeros((RUNS, KMAX, 2), np.float64)
pad[:, :K] = starts
cent_d = torch.empty((RUNS, KMAX, 2), dtype=torch.float64, device=dev)
start_d = torch.from_numpy(pad).to(dev)


def device_call(max_iter):
    """-> seconds of one call (it synchronises the stream itself)"""
    cent_d.copy_(start_d)
    torch.cuda.synchronize()
    t = time.perf_counter()
    X.call("myolo_anchor_kmeans", X.ptr(wh_d), N, run_k.ctypes.data, X.ptr(cent_d), RUNS, max_iter, X.ptr(counts), X.ptr(iters), X.ptr(conv),
           X.ptr(miou), None, X.ptr(ws), ws.numel(), X.stream())
    return time.perf_counter() - t


# ---- host: one pass of run r over points [lo, hi) -> integer sums and counts
w64, h64 = wh[:, 0].astype(np.float64), wh[:, 1].astype(np.float64)


def host_part(cent, lo, hi):
    sums, cnt = np.zeros((K, 2), np.int64), np.zeros(K, np.int64)
    cw, ch = cent[:, 0][None, :], cent[:, 1][None, :]
    for a in range(lo, hi, CHUNK):
        w, h = w64[a:min(a + CHUNK, hi), None], h64[a:min(a + CHUNK, hi), None]
        inter = np.minimum(w, cw) * np.minimum(h, ch)
        assign = np.argmin(1.0 - inter / ((w * h + cw * ch) - inter), axis=1)
        cnt += np.bincount(assign, minlength=K)
        sums[:, 0] += np.bincount(assign, weights=w[:, 0], minlength=K).astype(np.int64)      # (sums far below 2^53: exact)
        sums[:, 1] += np.bincount(assign, weights=h[:, 0], minlength=K).astype(np.int64)
    return sums, cnt


def host_passes(passes):
    cent = starts.copy()
    halves = [(0, N // 2), (N // 2, N)]
    with ThreadPoolExecutor(THREADS) as ex:
        t = time.perf_counter()
        for _ in range(passes):
            parts = list(ex.map(lambda rc: host_part(cent[rc[0]], *halves[rc[1]]), [(r, c) for r in range(RUNS) for c in range(2)]))
            for r in range(RUNS):
                sums, cnt = parts[2 * r][0] + parts[2 * r + 1][0], parts[2 * r][1] + parts[2 * r + 1][1]
                full = cnt > 0
                cent[r][full] = sums[full] / cnt[full][:, None]
        return time.perf_counter() - t, cent


device_call(HOST_PASSES)                                          # also the warm-up: code objects, clocks
host_s, host_cent = host_passes(HOST_PASSES)
same = cent_d.cpu().numpy()[:, :K].tobytes() == host_cent.tobytes()
assert same, "the device's centroids after %d passes differ from the host restatement's" % HOST_PASSES
device_call(300)
first = int(iters.min().item())                                   # the passes of the run that stops first: every timed call stays below them
LONG = min(LONG, first - 1)
assert LONG - SHORT >= 16, "the first run stops after %d passes: too few to time" % first
for _ in range(2):
    device_call(LONG)
ms = []
for _ in range(REPS):
    a, b = device_call(SHORT), device_call(LONG)
    assert int(iters.min().item()) == LONG, "a run converged within %d passes: the difference does not count %d passes" % (LONG, LONG - SHORT)
    ms.append(1e3 * (b - a) / (LONG - SHORT))
res = {"n": N, "k": K, "runs": RUNS, "device_ms_per_pass_repetitions": ms, "device_ms_per_pass_median": float(np.median(ms)),
       "spread_max_over_min": float(max(ms) / min(ms)), "passes_short_long": [SHORT, LONG], "passes_of_the_first_run_to_stop": first,
       "host_threads": THREADS, "host_passes_timed": HOST_PASSES, "host_ms_per_pass": 1e3 * host_s / HOST_PASSES,
       "host_over_device": 1e3 * host_s / HOST_PASSES / float(np.median(ms)), "centroids_equal_after_host_passes": bool(same)}
print(json.dumps(res))
assert res["host_over_device"] >= 1.0, "the device is slower than the host restatement"
