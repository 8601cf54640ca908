// Segment rasteriser (myolo/coco.py and myolo/via.py datasets through Net.stage_segments, MaskYOLO.evaluate and anchors.dataset_boxes): decodes the
// annotations of a batch straight into the [B,H,W,T] instance masks the device augmenter and the overlap counter read.  A slot holds any number of
// polygon parts, whose fills are OR-ed, and / or one run-length code (a VIA outline is a slot of one part); no mask is built on the host or
// crosses PCIe.
//
// A part is filled as skimage.draw.polygon fills it (scikit-image 0.18.3, restated in myolo/polygon.py): for pixel (y, x) walk the vertices
// cyclically, count the edges that cross the pixel's row to its right and to its left, and take the pixel when either count is odd or the pixel
// sits on a vertex.  The arithmetic is a contract: x1*y0, x0*y1, their difference and the quotient by (y0 - y1) are four
// IEEE binary64 operations in that order.  This unit is compiled with -ffp-contract=off and asks for it again here: with float vertices a fused
// multiply-add can flip the sign of x1*y0 - x0*y1 for a pixel next to an edge.  A run-length code is
// given by its boundaries (the running sums of its counts without the final total): pixel (r, c) of a source image of height h sits at
// p = c * h + r and is set when the number of boundaries <= p is odd.  Integer work: exact, and zero-length runs (equal boundaries) cancel.
#include "myolo_common.h"
#include <limits.h>
#pragma clang fp contract(off)

#define SEG_THREADS 256
#define SEG_WAVES (SEG_THREADS / 64)
#define SEG_CHUNK 256        // vertices of one part staged in LDS at a time (tests/golden/polygon_fixture.npz records it: outlines of CHUNK-1, CHUNK, CHUNK+1)
#define SEG_GROUP 32         // instance slots whose bits a lane gathers in one register; also the parts whose row extents are formed at a time
#define SEG_EPS 1e-12

__device__ __forceinline__ double seg_wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// A workgroup owns SEG_WAVES consecutive output rows x 64 consecutive output columns of one image, one wave per row, so
// the source row y and both straddle tests are wave-uniform.  Per group of up to SEG_GROUP slots:
//   (A) the group's parts are consecutive in part_off (slot_part ascends); they are taken SEG_GROUP at a time: (1) wave w derives the row extent
//       [min r, max r] of parts w, w + SEG_WAVES, ... from one coalesced read; (2) a part none of the workgroup's rows can meet is skipped by the
//       whole workgroup, and a wave whose row cannot meet it sits the vertex loop out; (3) the vertices go through LDS in chunks of SEG_CHUNK.
//       Every part starts its own x0, y0, parities and vertex flag, and its result is OR-ed into its slot's bit;
//   (B) a slot with boundaries: each lane searches its p among them (upper bound; the lanes of a wave are h apart) and ORs the parity in;
//   (C) each lane stores the group's bytes of its pixel, consecutive lanes writing consecutive runs of T bytes;
//   (D) with box_acc, lane 0 of a wave folds the columns its row sets into the slot's box with integer atomicMin / atomicMax: the result does not
//       depend on the order the waves arrive in.
__global__ __launch_bounds__(SEG_THREADS) void segment_masks_kernel(const double* __restrict__ verts, const int32_t* __restrict__ part_off,
                                                                    const int32_t* __restrict__ slot_part, const int32_t* __restrict__ bounds,
                                                                    const int32_t* __restrict__ slot_bound, const int32_t* __restrict__ src_h,
                                                                    const int32_t* __restrict__ src_row, const int32_t* __restrict__ src_col,
                                                                    uint8_t* __restrict__ masks, int32_t* __restrict__ box_acc, int H, int W, int T,
                                                                    int vec)
{
    __shared__ double s_v[SEG_CHUNK * 2];
    __shared__ double s_lo[SEG_GROUP], s_hi[SEG_GROUP];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = blockIdx.y * SEG_WAVES + wave, col = blockIdx.x * 64 + lane;
    const bool row_ok = row < H, live = row_ok && col < W;
    // (a wave or lane past the frame computes on the last row / column and stores nothing: every wave reaches every barrier)
    const int yi = src_row[(long long)b * H + (row_ok ? row : H - 1)];
    const int xi = src_col[(long long)b * W + (col < W ? col : W - 1)];
    const double y = (double)yi, x = (double)xi;
    // the pixel's place in a column-major run-length code (h * w < 2^31 where the image has one; unsigned: no overflow is undefined where it has none)
    const int pos = (int)((unsigned)xi * (unsigned)src_h[b] + (unsigned)yi);
    const int row_first = blockIdx.y * SEG_WAVES, row_last = min(row_first + SEG_WAVES, H) - 1;
    // the workgroup's source rows span [ya, yb] whichever way the table runs
    double ya = (double)src_row[(long long)b * H + row_first], yb = ya;
    for (int rr = row_first + 1; rr <= row_last; ++rr) {
        const double v = (double)src_row[(long long)b * H + rr];
        ya = fmin(ya, v); yb = fmax(yb, v);
    }
    uint8_t* out = masks + (((long long)b * H + (row_ok ? row : 0)) * W + (col < W ? col : 0)) * T;
    const int32_t* sp = slot_part + (long long)b * T;
    const int32_t* sb = slot_bound + (long long)b * T;

    for (int t0 = 0; t0 < T; t0 += SEG_GROUP) {
        const int nt = min(SEG_GROUP, T - t0);
        uint32_t bits = 0;
        // (A) the polygon parts of slots t0 .. t0 + nt - 1
        const int p_end = sp[t0 + nt];
        int k = 0;                                              // the slot of the part in hand (workgroup-uniform)
        for (int p0 = sp[t0]; p0 < p_end; p0 += SEG_GROUP) {
            const int np = min(SEG_GROUP, p_end - p0);
            for (int j = wave; j < np; j += SEG_WAVES) {
                const int v0 = part_off[p0 + j], n = part_off[p0 + j + 1] - v0;
                double lo = INFINITY, hi = -INFINITY;
                for (int i = lane; i < n; i += 64) {
                    const double r = verts[2 * (long long)(v0 + i)];
                    lo = fmin(lo, r); hi = fmax(hi, r);
                }
                lo = seg_wave_min(lo); hi = -seg_wave_min(-hi);
                if (lane == 0) { s_lo[j] = lo; s_hi[j] = hi; }
            }
            __syncthreads();
            for (int j = 0; j < np; ++j) {
                while (p0 + j >= sp[t0 + k + 1]) ++k;           // (p0 + j < sp[t0 + nt]: k stays below nt)
                const int v0 = part_off[p0 + j], n = part_off[p0 + j + 1] - v0;
                const double lo = s_lo[j], hi = s_hi[j];
                // every r[i] - y of a row is >= lo - y and <= hi - y (rounding is monotonic): when all of them are >= eps, or all <= -eps, no vertex
                // test and no straddle test can hold on that row.  A part without vertices has lo = +inf.
                if (n <= 0 || lo - yb >= SEG_EPS || hi - ya <= -SEG_EPS) continue;         // the whole workgroup: no barrier is skipped by a part of it
                const bool mine = !(lo - y >= SEG_EPS || hi - y <= -SEG_EPS);             // wave-uniform
                const double* pv = verts + 2 * (long long)v0;
                double y0 = pv[2 * (long long)(n - 1)] - y, x0 = pv[2 * (long long)(n - 1) + 1] - x;   // the previous vertex of vertex 0 is the last one
                bool rc = false, lc = false, vt = false;
                for (int c0 = 0; c0 < n; c0 += SEG_CHUNK) {
                    const int m = min(SEG_CHUNK, n - c0);
                    __syncthreads();                                                       // the previous chunk has been read
                    for (int i = tid; i < 2 * m; i += SEG_THREADS) s_v[i] = pv[2 * (long long)c0 + i];
                    __syncthreads();
                    if (mine) {
                        for (int i = 0; i < m; ++i) {
                            const double y1 = s_v[2 * i] - y, x1 = s_v[2 * i + 1] - x;
                            if (fabs(y1) < SEG_EPS && fabs(x1) < SEG_EPS) vt = true;
                            const bool sr = (y1 > 0.0) != (y0 > 0.0), sl = (y1 < 0.0) != (y0 < 0.0);
                            if (sr || sl) {                                                // wave-uniform: y1 and y0 are
                                const double q = (x1 * y0 - x0 * y1) / (y0 - y1);
                                if (sr && q > 0.0) rc = !rc;
                                if (sl && q < 0.0) lc = !lc;
                            }
                            x0 = x1; y0 = y1;
                        }
                    }
                }
                if (vt || rc || lc) bits |= 1u << k;
            }
            __syncthreads();                                    // s_lo / s_hi are rewritten by the next parts
        }
        // (B) the run-length codes of the group
        for (int kk = 0; kk < nt; ++kk) {
            const int b0 = sb[t0 + kk], nb = sb[t0 + kk + 1] - b0;
            if (nb <= 0) continue;                              // wave-uniform
            const int32_t* bd = bounds + b0;
            int lo = 0, hi = nb;                                // the number of boundaries <= pos
            while (lo < hi) {
                const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                if (bd[mid] <= pos) lo = mid + 1; else hi = mid;
            }
            bits |= (uint32_t)(lo & 1) << kk;
        }
        // (C) the group's bytes of this pixel
        if (live) {
            uint8_t* p = out + t0;
            if (vec == 4) {                                    // T % 4 == 0 and a word-aligned base: t0 and nt are multiples of 4
                for (int kk = 0; kk < nt; kk += 4) {
                    const uint32_t q = bits >> kk;
                    *(uint32_t*)(p + kk) = (q & 1u) | ((q & 2u) << 7) | ((q & 4u) << 14) | ((q & 8u) << 21);
                }
            } else if (vec == 2) {                             // T % 2 == 0 and a halfword-aligned base
                for (int kk = 0; kk < nt; kk += 2) {
                    const uint32_t q = bits >> kk;
                    *(uint16_t*)(p + kk) = (uint16_t)((q & 1u) | ((q & 2u) << 7));
                }
            } else {
                for (int kk = 0; kk < nt; ++kk) p[kk] = (uint8_t)((bits >> kk) & 1u);
            }
        }
        // (D) the group's boxes: this wave's row and the first / last column it sets
        if (box_acc) {
            const uint32_t mine_bits = live ? bits : 0u;
            for (int kk = 0; kk < nt; ++kk) {
                const unsigned long long set = __ballot((mine_bits >> kk) & 1u);
                if (set != 0ull && lane == 0) {
                    int32_t* q = box_acc + ((long long)b * T + t0 + kk) * 4;
                    const int c_base = blockIdx.x * 64;
                    atomicMin(q + 0, c_base + (__ffsll((long long)set) - 1));
                    atomicMin(q + 1, row);
                    atomicMax(q + 2, c_base + (63 - __clzll((long long)set)) + 1);
                    atomicMax(q + 3, row + 1);
                }
            }
        }
    }
}

// boxes before the fill: x1 = y1 = INT_MAX, x2 = y2 = 0 (any set pixel makes x2 >= 1)
__global__ void segment_boxes_init_kernel(int32_t* __restrict__ boxes, long long n_slots)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots * 4) boxes[i] = (i & 2) ? 0 : INT_MAX;
}

// ... and after it: a slot no pixel of which is set reads 0, 0, 0, 0
__global__ void segment_boxes_finish_kernel(int32_t* __restrict__ boxes, long long n_slots)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots && boxes[4 * i + 2] == 0) { boxes[4 * i] = 0; boxes[4 * i + 1] = 0; boxes[4 * i + 3] = 0; }
}

extern "C" {

int myolo_segment_masks(const double* verts, const int32_t* part_off, const int32_t* slot_part, const int32_t* bounds, const int32_t* slot_bound,
                        const int32_t* src_h, const int32_t* src_row, const int32_t* src_col, uint8_t* masks, int32_t* boxes,
                        int B, int H, int W, int T, void* stream)
{
    // (verts may be NULL when no slot has a part, bounds when none has a run-length code, boxes when no box is wanted)
    MYOLO_REQUIRE(part_off && slot_part && slot_bound && src_h && src_row && src_col && masks, "segment_masks: null pointer");
    MYOLO_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && T > 0, "segment_masks: bad sizes (B=%d, H=%d, W=%d, T=%d)", B, H, W, T);
    MYOLO_REQUIRE((H + SEG_WAVES - 1) / SEG_WAVES <= 65535, "segment_masks: H=%d exceeds %d rows", H, 65535 * SEG_WAVES);
    MYOLO_REQUIRE((long long)B * T < (1ll << 31) - 1, "segment_masks: B * T = %lld slots exceed the int32 offsets", (long long)B * T);
    const hipStream_t s = (hipStream_t)stream;
    const long long n_slots = (long long)B * T;
    const unsigned box_blocks4 = (unsigned)((n_slots * 4 + 255) / 256), box_blocks = (unsigned)((n_slots + 255) / 256);
    if (boxes) {
        hipLaunchKernelGGL(segment_boxes_init_kernel, dim3(box_blocks4), dim3(256), 0, s, boxes, n_slots);
        MYOLO_CHECK_LAUNCH();
    }
    const int vec = (T % 4 == 0 && ((uintptr_t)masks & 3) == 0) ? 4 : (T % 2 == 0 && ((uintptr_t)masks & 1) == 0) ? 2 : 1;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + SEG_WAVES - 1) / SEG_WAVES), (unsigned)B);
    hipLaunchKernelGGL(segment_masks_kernel, grid, dim3(SEG_THREADS), 0, s, verts, part_off, slot_part, bounds, slot_bound, src_h, src_row, src_col,
                       masks, boxes, H, W, T, vec);
    MYOLO_CHECK_LAUNCH();
    if (boxes) {
        hipLaunchKernelGGL(segment_boxes_finish_kernel, dim3(box_blocks), dim3(256), 0, s, boxes, n_slots);
        MYOLO_CHECK_LAUNCH();
    }
    return MYOLO_OK;
}

}  // extern "C"
