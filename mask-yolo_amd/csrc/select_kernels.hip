// detect()'s selection of a batch on the device (myolo/detect.py: select / Selection; contract: DESIGN.md section 23): per image the rows with
// area, the first K of them by score, those at or above the confidence threshold, and the all-pairs same-class suppression of myolo_utils.NMB --
// every decision the bits the host takes.  One workgroup per image; nothing leaves the device but sel / picked / count.
//
// The arithmetic is restated operation for operation, which is why this unit is compiled with -ffp-contract=off and asks for it again:
//     live:  (x2 - x1) * (y2 - y1) > 0                                     in binary32
//     order: descending score, ties by HIGHER row first                    (np.argsort(scores, kind="stable")[::-1] on the live rows)
//     keep:  (double)score >= cs_threshold
//     iou:   corners (double)x * shape0, (double)y * shape1; _interval_overlap's branches as written; inter / ((w1*h1 + w2*h2) - inter)
// The order is a bitonic sort of 64-bit keys in LDS: the score's bits mapped monotone in the high word (-0 counts as +0, as it compares), the
// row in the low word; a row without area has key 0, below every finite score's key.  4096 keys are 32 KB.
#include "myolo_common.h"
#pragma clang fp contract(off)

#define SEL_THREADS 256
#define SEL_MAXK 128
#define SEL_MAXR 4096

static_assert(SEL_MAXK <= SEL_THREADS, "one thread per slot");

__device__ __forceinline__ double sel_min(double a, double b) { return b < a ? b : a; }     // Python's min(a, b)

// myolo_utils._interval_overlap([x1, x2], [x3, x4])
__device__ __forceinline__ double sel_interval_overlap(double x1, double x2, double x3, double x4)
{
    if (x3 < x1) {
        if (x4 < x1) return 0.0;
        return sel_min(x2, x4) - x1;
    }
    if (x2 < x3) return 0.0;
    return sel_min(x2, x4) - x3;
}

__global__ __launch_bounds__(SEL_THREADS) void select_detections_kernel(const float* __restrict__ det, int R, int n_live, int K, int n2,
                                                                        double cs_threshold, double nms_threshold, double shape0, double shape1,
                                                                        int32_t* __restrict__ sel, float* __restrict__ picked,
                                                                        int32_t* __restrict__ count)
{
    __shared__ unsigned long long s_key[SEL_MAXR];
    __shared__ double s_x1[SEL_MAXK], s_y1[SEL_MAXK], s_x2[SEL_MAXK], s_y2[SEL_MAXK];
    __shared__ int s_cls[SEL_MAXK], s_row[SEL_MAXK], s_flag[SEL_MAXK], s_drop[SEL_MAXK];

    const int b = blockIdx.x, t = threadIdx.x;
    const float* __restrict__ d = det + (size_t)b * (size_t)R * 6;
    int32_t* __restrict__ sel_b = sel + (size_t)b * (size_t)K;
    uint32_t* __restrict__ picked_b = reinterpret_cast<uint32_t*>(picked) + (size_t)b * (size_t)K * 6;

    if (b >= n_live) {                                          // a padding image (the whole workgroup: before any barrier)
        if (t < K) {
            sel_b[t] = -1;
            for (int c = 0; c < 6; ++c) picked_b[(size_t)t * 6 + c] = 0u;
        }
        if (t == 0) count[b] = 0;
        return;
    }

    // 1. keys of the live rows, 0 for the others and for the padding up to the power of two
    for (int r = t; r < n2; r += SEL_THREADS) {
        unsigned long long key = 0ull;
        if (r < R) {
            const float x1 = d[(size_t)r * 6 + 0], y1 = d[(size_t)r * 6 + 1], x2 = d[(size_t)r * 6 + 2], y2 = d[(size_t)r * 6 + 3];
            const float w = x2 - x1, h = y2 - y1;
            const float area = w * h;
            if (area > 0.0f) {
                const float score = d[(size_t)r * 6 + 4];
                uint32_t u = score == 0.0f ? 0u : __float_as_uint(score);
                u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                key = ((unsigned long long)u << 32) | (unsigned long long)(uint32_t)r;
            }
        }
        s_key[r] = key;
    }
    __syncthreads();

    // 2. bitonic sort, descending
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < n2; i += SEL_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long a = s_key[i], c = s_key[p];
                    const bool descending = (i & k) == 0;
                    if (descending ? (a < c) : (a > c)) {
                        s_key[i] = c;
                        s_key[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }

    // 3. the first K live rows; of those, the ones at or above the threshold, in order: the list L
    int row = -1, flag = 0;
    if (t < K) {
        const unsigned long long key = t < n2 ? s_key[t] : 0ull;
        if (key != 0ull) {
            row = (int)(uint32_t)(key & 0xFFFFFFFFull);
            flag = (double)d[(size_t)row * 6 + 4] >= cs_threshold ? 1 : 0;
        }
        s_flag[t] = flag;
    }
    __syncthreads();
    int nL = 0;
    for (int j = 0; j < K; ++j) nL += s_flag[j];                // (broadcast reads)
    if (flag) {
        int pos = 0;
        for (int j = 0; j < t; ++j) pos += s_flag[j];
        s_x1[pos] = (double)d[(size_t)row * 6 + 0] * shape0;
        s_y1[pos] = (double)d[(size_t)row * 6 + 1] * shape1;
        s_x2[pos] = (double)d[(size_t)row * 6 + 2] * shape0;
        s_y2[pos] = (double)d[(size_t)row * 6 + 3] * shape1;
        s_cls[pos] = (int)d[(size_t)row * 6 + 5];
        s_row[pos] = row;
        s_drop[pos] = 0;
    }
    __syncthreads();

    // 4. NMB over all pairs i < j of L: j is dropped by ANY earlier i of its class, dropped or not (every writer stores the same 1)
    for (int p = t; p < nL * nL; p += SEL_THREADS) {
        const int i = p / nL, j = p - i * nL;
        if (i < j && s_cls[i] == s_cls[j]) {
            const double ax1 = s_x1[i], ay1 = s_y1[i], ax2 = s_x2[i], ay2 = s_y2[i];
            const double bx1 = s_x1[j], by1 = s_y1[j], bx2 = s_x2[j], by2 = s_y2[j];
            const double iw = sel_interval_overlap(ax1, ax2, bx1, bx2);
            const double ih = sel_interval_overlap(ay1, ay2, by1, by2);
            const double inter = iw * ih;
            const double w1 = ax2 - ax1, h1 = ay2 - ay1, w2 = bx2 - bx1, h2 = by2 - by1;
            const double a1 = w1 * h1, a2 = w2 * h2;
            const double den = (a1 + a2) - inter;
            if (den != 0.0) {                                   // (the host raises on a zero denominator: outside the contract)
                const double iou = inter / den;
                if (iou >= nms_threshold) s_drop[j] = 1;
            }
        }
    }
    __syncthreads();

    // 5. the survivors, in order
    int n_out = 0;
    for (int j = 0; j < nL; ++j) n_out += s_drop[j] ? 0 : 1;
    if (t < nL && !s_drop[t]) {
        int pos = 0;
        for (int j = 0; j < t; ++j) pos += s_drop[j] ? 0 : 1;
        const int r = s_row[t];
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(d) + (size_t)r * 6;
        sel_b[pos] = r;
        for (int c = 0; c < 6; ++c) picked_b[(size_t)pos * 6 + c] = src[c];
    }
    if (t >= n_out && t < K) {
        sel_b[t] = -1;
        for (int c = 0; c < 6; ++c) picked_b[(size_t)t * 6 + c] = 0u;
    }
    if (t == 0) count[b] = n_out;
}

extern "C" {

int myolo_select_detections(const float* det, int B, int R, int n_live, int K, double cs_threshold, double nms_threshold, int shape0, int shape1,
                            int32_t* sel, float* picked, int32_t* count, void* stream)
{
    MYOLO_REQUIRE(det && sel && picked && count, "select_detections: null pointer");
    MYOLO_REQUIRE(B >= 1, "select_detections: need B >= 1 (got B=%d)", B);
    MYOLO_REQUIRE(K >= 1 && K <= SEL_MAXK, "select_detections: need 1 <= K <= %d (got K=%d)", SEL_MAXK, K);
    MYOLO_REQUIRE(R >= 1 && R <= SEL_MAXR, "select_detections: need 1 <= R <= %d (got R=%d)", SEL_MAXR, R);
    MYOLO_REQUIRE(n_live >= 0 && n_live <= B, "select_detections: need 0 <= n_live <= B (got n_live=%d, B=%d)", n_live, B);
    int n2 = 2;
    while (n2 < R) n2 <<= 1;
    hipLaunchKernelGGL(select_detections_kernel, dim3((unsigned)B), dim3(SEL_THREADS), 0, (hipStream_t)stream, det, R, n_live, K, n2, cs_threshold,
                       nms_threshold, (double)shape0, (double)shape1, sel, picked, count);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

}  // extern "C"
