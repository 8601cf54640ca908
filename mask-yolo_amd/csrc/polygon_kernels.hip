// Polygon rasteriser (myolo/via.py datasets through Net.stage_polygons): fills the outlines of a batch straight into the [B,H,W,T] instance masks
// the device augmenter reads, so that no mask is built on the host or crosses PCIe.  The fill is skimage.draw.polygon's (scikit-image 0.18.3,
// restated in myolo/polygon.py): for pixel (y, x) walk the vertices cyclically, count the edges that cross the pixel's row to its right and to its
// left, and take the pixel when either count is odd or the pixel sits on a vertex.
//
// The arithmetic is a contract ("Polygon annotations"): x1*y0, x0*y1, their difference and the quotient by (y0 - y1) are four IEEE
// binary64 operations in that order.  This unit is compiled with -ffp-contract=off and asks for it again here: with float vertices a fused
// multiply-add can flip the sign of x1*y0 - x0*y1 for a pixel next to an edge.
#include "myolo_common.h"
#pragma clang fp contract(off)

#define POLY_THREADS 256
#define POLY_WAVES (POLY_THREADS / 64)
#define POLY_CHUNK 256       // vertices of one polygon staged in LDS at a time (tests/golden/polygon_fixture.npz records it: outlines of CHUNK-1, CHUNK, CHUNK+1)
#define POLY_GROUP 32        // instance slots whose bits a lane gathers in one register before it stores their bytes
#define POLY_EPS 1e-12

__device__ __forceinline__ double poly_wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// A workgroup owns POLY_WAVES consecutive output rows x 64 consecutive output columns of one image; wave w owns row blockIdx.y * POLY_WAVES + w, so
// the source row y is the same in every lane and the two straddle tests below are the same in every lane: only the one or two edges that cross
// the row reach the divide.  Per group of up to POLY_GROUP slots: (1) the waves derive each polygon's [min r, max r] from one coalesced read of its
// row coordinates; (2) a slot none of the workgroup's rows can meet is skipped by the whole workgroup, and a wave whose row cannot meet it sits the
// vertex loop out; (3) the vertices go through LDS in chunks of POLY_CHUNK, and x0, y0 and the two parities are carried from chunk to chunk in
// registers; (4) each lane stores the group's bytes of its pixel, consecutive lanes writing consecutive runs of T bytes.
__global__ __launch_bounds__(POLY_THREADS) void polygon_masks_kernel(const double* __restrict__ verts, const int32_t* __restrict__ poly_off,
                                                                     const int32_t* __restrict__ src_row, const int32_t* __restrict__ src_col,
                                                                     uint8_t* __restrict__ masks, int H, int W, int T, int vec)
{
    __shared__ double s_v[POLY_CHUNK * 2];
    __shared__ double s_lo[POLY_GROUP], s_hi[POLY_GROUP];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = blockIdx.y * POLY_WAVES + wave, col = blockIdx.x * 64 + lane;
    const bool row_ok = row < H, live = row_ok && col < W;
    // (a wave or lane past the frame computes on the last row / column and stores nothing: every wave reaches every barrier)
    const double y = (double)src_row[(long long)b * H + (row_ok ? row : H - 1)];
    const double x = (double)src_col[(long long)b * W + (col < W ? col : W - 1)];
    const int row_first = blockIdx.y * POLY_WAVES, row_last = min(row_first + POLY_WAVES, H) - 1;
    // the workgroup's source rows span [ya, yb] whichever way the table runs
    double ya = (double)src_row[(long long)b * H + row_first], yb = ya;
    for (int rr = row_first + 1; rr <= row_last; ++rr) {
        const double v = (double)src_row[(long long)b * H + rr];
        ya = fmin(ya, v); yb = fmax(yb, v);
    }
    uint8_t* out = masks + (((long long)b * H + (row_ok ? row : 0)) * W + (col < W ? col : 0)) * T;
    const int32_t* off = poly_off + (long long)b * T;

    for (int t0 = 0; t0 < T; t0 += POLY_GROUP) {
        const int nt = min(POLY_GROUP, T - t0);
        // (1) row extent of each polygon of the group: wave w takes slots w, w + POLY_WAVES, ...
        for (int k = wave; k < nt; k += POLY_WAVES) {
            const int v0 = off[t0 + k], n = off[t0 + k + 1] - v0;
            double lo = INFINITY, hi = -INFINITY;
            for (int i = lane; i < n; i += 64) {
                const double r = verts[2 * (long long)(v0 + i)];
                lo = fmin(lo, r); hi = fmax(hi, r);
            }
            lo = poly_wave_min(lo); hi = -poly_wave_min(-hi);
            if (lane == 0) { s_lo[k] = lo; s_hi[k] = hi; }
        }
        __syncthreads();
        uint32_t bits = 0;
        for (int k = 0; k < nt; ++k) {
            const int v0 = off[t0 + k], n = off[t0 + k + 1] - v0;
            const double lo = s_lo[k], hi = s_hi[k];
            // every r[i] - y of a row is >= lo - y and <= hi - y (rounding is monotonic): when all of them are >= eps, or all <= -eps, no vertex
            // test and no straddle test can hold on that row.  An empty slot has lo = +inf.
            if (n <= 0 || lo - yb >= POLY_EPS || hi - ya <= -POLY_EPS) continue;           // the whole workgroup: no barrier is skipped by a part of it
            const bool mine = !(lo - y >= POLY_EPS || hi - y <= -POLY_EPS);               // wave-uniform
            const double* pv = verts + 2 * (long long)v0;
            double y0 = pv[2 * (long long)(n - 1)] - y, x0 = pv[2 * (long long)(n - 1) + 1] - x;   // the previous vertex of vertex 0 is the last one
            bool rc = false, lc = false, vt = false;
            for (int c0 = 0; c0 < n; c0 += POLY_CHUNK) {
                const int m = min(POLY_CHUNK, n - c0);
                __syncthreads();                                                           // the previous chunk has been read
                for (int i = tid; i < 2 * m; i += POLY_THREADS) s_v[i] = pv[2 * (long long)c0 + i];
                __syncthreads();
                if (mine) {
                    for (int i = 0; i < m; ++i) {
                        const double y1 = s_v[2 * i] - y, x1 = s_v[2 * i + 1] - x;
                        if (fabs(y1) < POLY_EPS && fabs(x1) < POLY_EPS) vt = true;
                        const bool sr = (y1 > 0.0) != (y0 > 0.0), sl = (y1 < 0.0) != (y0 < 0.0);
                        if (sr || sl) {                                                    // wave-uniform: y1 and y0 are
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
        // (4) the group's bytes of this pixel
        if (live) {
            uint8_t* p = out + t0;
            if (vec == 4) {                                    // T % 4 == 0 and a word-aligned base: t0 and nt are multiples of 4
                for (int k = 0; k < nt; k += 4) {
                    const uint32_t q = bits >> k;
                    *(uint32_t*)(p + k) = (q & 1u) | ((q & 2u) << 7) | ((q & 4u) << 14) | ((q & 8u) << 21);
                }
            } else if (vec == 2) {                             // T % 2 == 0 and a halfword-aligned base
                for (int k = 0; k < nt; k += 2) {
                    const uint32_t q = bits >> k;
                    *(uint16_t*)(p + k) = (uint16_t)((q & 1u) | ((q & 2u) << 7));
                }
            } else {
                for (int k = 0; k < nt; ++k) p[k] = (uint8_t)((bits >> k) & 1u);
            }
        }
        __syncthreads();                                       // s_lo / s_hi are rewritten by the next group
    }
}

extern "C" {

int myolo_polygon_masks(const double* verts, const int32_t* poly_off, const int32_t* src_row, const int32_t* src_col, uint8_t* masks,
                        int B, int H, int W, int T, void* stream)
{
    MYOLO_REQUIRE(poly_off && src_row && src_col && masks, "polygon_masks: null pointer");          // (verts may be NULL when every slot is empty)
    MYOLO_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && T > 0, "polygon_masks: bad sizes (B=%d, H=%d, W=%d, T=%d)", B, H, W, T);
    MYOLO_REQUIRE((H + POLY_WAVES - 1) / POLY_WAVES <= 65535, "polygon_masks: H=%d exceeds %d rows", H, 65535 * POLY_WAVES);
    MYOLO_REQUIRE((long long)B * T < (1ll << 31) - 1, "polygon_masks: B * T = %lld slots exceed the int32 offsets", (long long)B * T);
    const int vec = (T % 4 == 0 && ((uintptr_t)masks & 3) == 0) ? 4 : (T % 2 == 0 && ((uintptr_t)masks & 1) == 0) ? 2 : 1;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + POLY_WAVES - 1) / POLY_WAVES), (unsigned)B);
    hipLaunchKernelGGL(polygon_masks_kernel, grid, dim3(POLY_THREADS), 0, (hipStream_t)stream, verts, poly_off, src_row, src_col, masks, H, W, T, vec);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

}  // extern "C"
