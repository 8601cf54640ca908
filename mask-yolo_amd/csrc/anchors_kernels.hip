// Anchor fitting (myolo/anchors.py: kmeans_anchors / sweep_anchors): batched k-means over box sizes (w, h) with 1 - IoU as the distance, the
// YOLO-v2 recipe of the reference's example/*/03_anchor_generator.ipynb.  `runs` independent runs -- the restarts of one k, or a sweep over k --
// go through ONE call: blockIdx.y is the run, every run has its own k <= 32 and its own centroids.
//
// The arithmetic is binary64 without contraction, in this order (which is why this unit is compiled with -ffp-contract=off and asks for it again):
//     inter = min(w, cw) * min(h, ch);   iou = inter / ((w * h + cw * ch) - inter);   d = 1.0 - iou;   assignment = lowest index of the smallest d
// The per-cluster sums are 64-bit INTEGERS (LDS atomics per wave, then one global atomic per workgroup and cluster): exact, so the order the
// workgroups arrive in cannot show and two calls give the same bits.  No floating-point atomic anywhere in this file: the mean IoU is summed from
// per-workgroup partials in index order.
//
// The loop over passes is the host's: one assign launch and one update launch per pass.  A finished run's workgroups return on its device flag;
// the host reads the flags every ANCH_POLL passes and stops launching when all are set.  Nothing waits on another workgroup.
#include "myolo_common.h"
#include <vector>
#pragma clang fp contract(off)

#define ANCH_THREADS 256
#define ANCH_WAVES (ANCH_THREADS / 64)
#define ANCH_KMAX 32
#define ANCH_MAX_BLOCKS 1024      // workgroups per run (each strides over the points); also the partials of the mean IoU
#define ANCH_POINTS_PER_BLOCK 1024
#define ANCH_POLL 4               // passes between two reads of the runs' flags

static inline int anch_blocks(int64_t n)
{
    const int64_t b = cdiv64(n, ANCH_POINTS_PER_BLOCK);
    return (int)(b < 1 ? 1 : (b > ANCH_MAX_BLOCKS ? ANCH_MAX_BLOCKS : b));
}

// workspace: k [runs] int32 | done [runs] int32 | changed [runs] uint32 | sums [runs,32,3] uint64 | partial [runs,blocks] double | prev [runs,n] uint8
struct AnchWs {
    size_t k, done, changed, sums, partial, prev, total;
};

static AnchWs anch_plan(int64_t n, int runs)
{
    AnchWs p;
    size_t o = 0;
    p.k = o;       o += align256((size_t)runs * sizeof(int32_t));
    p.done = o;    o += align256((size_t)runs * sizeof(int32_t));
    p.changed = o; o += align256((size_t)runs * sizeof(uint32_t));
    p.sums = o;    o += align256((size_t)runs * ANCH_KMAX * 3 * sizeof(unsigned long long));
    p.partial = o; o += align256((size_t)runs * (size_t)anch_blocks(n) * sizeof(double));
    p.prev = o;    o += align256((size_t)runs * (size_t)n);
    p.total = o;
    return p;
}

// One assignment pass of every unfinished run.  A workgroup strides over the points: point i of every stride is read coalesced; k is uniform, so the
// centroids are LDS broadcasts.
__global__ __launch_bounds__(ANCH_THREADS) void anchor_assign_kernel(const int32_t* __restrict__ wh, long long n, const int32_t* __restrict__ run_k,
                                                                     const double* __restrict__ centroids, const int32_t* __restrict__ done,
                                                                     uint8_t* __restrict__ prev, unsigned long long* __restrict__ sums,
                                                                     unsigned int* __restrict__ changed)
{
    const int r = blockIdx.y;
    if (done[r]) return;                                        // the whole workgroup: before any barrier
    __shared__ double s_cw[ANCH_KMAX], s_ch[ANCH_KMAX], s_ca[ANCH_KMAX];
    __shared__ unsigned long long s_acc[ANCH_WAVES][ANCH_KMAX][3];
    __shared__ unsigned int s_changed;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int k = run_k[r];
    if (tid < k) {
        const double cw = centroids[((long long)r * ANCH_KMAX + tid) * 2], ch = centroids[((long long)r * ANCH_KMAX + tid) * 2 + 1];
        s_cw[tid] = cw; s_ch[tid] = ch; s_ca[tid] = cw * ch;
    }
    for (int i = tid; i < ANCH_WAVES * ANCH_KMAX * 3; i += ANCH_THREADS) (&s_acc[0][0][0])[i] = 0ull;
    if (tid == 0) s_changed = 0u;
    __syncthreads();

    uint8_t* pv = prev + (long long)r * n;
    unsigned int n_changed = 0;
    const long long step = (long long)gridDim.x * ANCH_THREADS;
    for (long long i = (long long)blockIdx.x * ANCH_THREADS + tid; i < n; i += step) {
        const int2 q = make_int2(wh[2 * i], wh[2 * i + 1]);
        const double w = (double)q.x, h = (double)q.y, a = w * h;
        int best = 0;
        double bd = 0.0;
        for (int j = 0; j < k; ++j) {
            const double inter = fmin(w, s_cw[j]) * fmin(h, s_ch[j]);
            const double iou = inter / ((a + s_ca[j]) - inter);
            const double d = 1.0 - iou;
            if (j == 0 || d < bd) { bd = d; best = j; }         // strict: the lowest index of the smallest d
        }
        if (pv[i] != (uint8_t)best) { ++n_changed; pv[i] = (uint8_t)best; }
        atomicAdd(&s_acc[wave][best][0], (unsigned long long)q.x);
        atomicAdd(&s_acc[wave][best][1], (unsigned long long)q.y);
        atomicAdd(&s_acc[wave][best][2], 1ull);
    }
    if (n_changed) atomicAdd(&s_changed, n_changed);
    __syncthreads();
    if (tid < k * 3) {
        const int j = tid / 3, c = tid - 3 * j;
        unsigned long long v = 0ull;
        for (int wv = 0; wv < ANCH_WAVES; ++wv) v += s_acc[wv][j][c];
        if (v) atomicAdd(&sums[((long long)r * ANCH_KMAX + j) * 3 + c], v);
    }
    if (tid == 0 && s_changed) atomicAdd(&changed[r], 1u);      // (the number of workgroups that saw a change: only != 0 matters)
}

// After a pass: one workgroup of ANCH_KMAX threads per run, thread j its cluster j.  Nothing changed: the run is converged and its centroids stay (they
// are the means of this assignment already).  Otherwise a non-empty cluster's centroid becomes (double)sum / (double)count and an EMPTY cluster keeps
// its centroid.  counts = the counts of the pass just made, so that they always belong to the assignment the workspace holds.
__global__ __launch_bounds__(ANCH_KMAX) void anchor_update_kernel(const int32_t* __restrict__ run_k, double* __restrict__ centroids,
                                                                  int32_t* __restrict__ done, unsigned long long* __restrict__ sums,
                                                                  unsigned int* __restrict__ changed, long long* __restrict__ counts,
                                                                  int32_t* __restrict__ iterations, int32_t* __restrict__ converged, int max_iter)
{
    const int r = blockIdx.x, j = threadIdx.x;
    if (done[r]) return;
    const int k = run_k[r];
    const unsigned int ch = changed[r];
    const int it = iterations[r] + 1;
    unsigned long long* s = sums + ((long long)r * ANCH_KMAX + j) * 3;
    const long long sw = (long long)s[0], sh = (long long)s[1], cnt = (long long)s[2];
    __syncthreads();                                            // everyone has read changed[r] / iterations[r]
    s[0] = 0ull; s[1] = 0ull; s[2] = 0ull;
    if (j < k) {
        counts[(long long)r * ANCH_KMAX + j] = cnt;
        if (ch != 0u && cnt > 0) {
            centroids[((long long)r * ANCH_KMAX + j) * 2] = (double)sw / (double)cnt;
            centroids[((long long)r * ANCH_KMAX + j) * 2 + 1] = (double)sh / (double)cnt;
        }
    }
    if (j == 0) {
        iterations[r] = it;
        changed[r] = 0u;
        if (ch == 0u) { converged[r] = 1; done[r] = 1; }
        else if (it >= max_iter) done[r] = 1;
    }
}

__device__ __forceinline__ double anch_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The final pass, against the final centroids: every point's largest IoU, summed per workgroup in a fixed order (a thread's points in index order,
// the butterfly of a wave, the waves in order) into partial[r, blockIdx.x]; assign = the last pass's assignment, widened.
__global__ __launch_bounds__(ANCH_THREADS) void anchor_score_kernel(const int32_t* __restrict__ wh, long long n, const int32_t* __restrict__ run_k,
                                                                    const double* __restrict__ centroids, const uint8_t* __restrict__ prev,
                                                                    double* __restrict__ partial, int32_t* __restrict__ assign)
{
    __shared__ double s_cw[ANCH_KMAX], s_ch[ANCH_KMAX], s_ca[ANCH_KMAX];
    __shared__ double s_part[ANCH_WAVES];
    const int r = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const int k = run_k[r];
    if (tid < k) {
        const double cw = centroids[((long long)r * ANCH_KMAX + tid) * 2], ch = centroids[((long long)r * ANCH_KMAX + tid) * 2 + 1];
        s_cw[tid] = cw; s_ch[tid] = ch; s_ca[tid] = cw * ch;
    }
    __syncthreads();
    const uint8_t* pv = prev + (long long)r * n;
    double acc = 0.0;
    const long long step = (long long)gridDim.x * ANCH_THREADS;
    for (long long i = (long long)blockIdx.x * ANCH_THREADS + tid; i < n; i += step) {
        const int2 q = make_int2(wh[2 * i], wh[2 * i + 1]);
        const double w = (double)q.x, h = (double)q.y, a = w * h;
        double m = 0.0;
        for (int j = 0; j < k; ++j) {
            const double inter = fmin(w, s_cw[j]) * fmin(h, s_ch[j]);
            const double iou = inter / ((a + s_ca[j]) - inter);
            if (j == 0 || iou > m) m = iou;
        }
        acc += m;
        if (assign) assign[(long long)r * n + i] = (int32_t)pv[i];
    }
    acc = anch_wave_sum(acc);
    if ((tid & 63) == 0) s_part[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = s_part[0];
        for (int wv = 1; wv < ANCH_WAVES; ++wv) t += s_part[wv];
        partial[(long long)r * gridDim.x + blockIdx.x] = t;
    }
}

// ... finished in index order by one thread per run
__global__ void anchor_finish_kernel(const double* __restrict__ partial, int blocks, long long n, double* __restrict__ mean_iou)
{
    if (threadIdx.x != 0) return;
    const int r = blockIdx.x;
    double t = 0.0;
    for (int b = 0; b < blocks; ++b) t += partial[(long long)r * blocks + b];
    mean_iou[r] = t / (double)n;
}

extern "C" {

size_t myolo_anchor_kmeans_ws_bytes(int64_t n, int runs)
{
    if (n < 1 || n > (1ll << 40) || runs < 1 || runs > 65535) return 0;
    return anch_plan(n, runs).total;
}

int myolo_anchor_kmeans(const int32_t* wh, int64_t n, const int32_t* run_k, double* centroids, int runs, int max_iter, int64_t* counts,
                        int32_t* iterations, int32_t* converged, double* mean_iou, int32_t* assign, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(wh && run_k && centroids && counts && iterations && converged && mean_iou && ws, "anchor_kmeans: null pointer");
    MYOLO_REQUIRE(n >= 1 && n <= (1ll << 40), "anchor_kmeans: n = %lld points (1 .. 2^40)", (long long)n);
    MYOLO_REQUIRE(runs >= 1 && runs <= 65535, "anchor_kmeans: runs = %d (1 .. 65535)", runs);
    MYOLO_REQUIRE(max_iter >= 1, "anchor_kmeans: max_iter = %d (>= 1)", max_iter);
    for (int r = 0; r < runs; ++r)
        MYOLO_REQUIRE(run_k[r] >= 1 && run_k[r] <= ANCH_KMAX, "anchor_kmeans: run %d has k = %d (1 .. %d)", r, run_k[r], ANCH_KMAX);
    const AnchWs p = anch_plan(n, runs);
    MYOLO_REQUIRE(ws_bytes >= p.total, "anchor_kmeans: workspace too small (%zu needed, %zu given)", p.total, ws_bytes);

    const hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    int32_t* d_k = (int32_t*)(base + p.k);
    int32_t* d_done = (int32_t*)(base + p.done);
    unsigned int* d_changed = (unsigned int*)(base + p.changed);
    unsigned long long* d_sums = (unsigned long long*)(base + p.sums);
    double* d_partial = (double*)(base + p.partial);
    uint8_t* d_prev = (uint8_t*)(base + p.prev);
    const int blocks = anch_blocks(n);

#define ANCH_HIP(call)                                                                          \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess) {                                                                \
            myolo_set_error("anchor_kmeans: %s failed: %s", #call, hipGetErrorString(e__));     \
            return MYOLO_ELAUNCH;                                                               \
        }                                                                                       \
    } while (0)

    ANCH_HIP(hipMemcpyAsync(d_k, run_k, (size_t)runs * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ANCH_HIP(hipMemsetAsync(base + p.done, 0, p.partial - p.done, s));                       // done, changed, sums
    ANCH_HIP(hipMemsetAsync(d_prev, 0xFF, (size_t)runs * (size_t)n, s));                     // no previous assignment
    ANCH_HIP(hipMemsetAsync(counts, 0, (size_t)runs * ANCH_KMAX * sizeof(int64_t), s));
    ANCH_HIP(hipMemsetAsync(iterations, 0, (size_t)runs * sizeof(int32_t), s));
    ANCH_HIP(hipMemsetAsync(converged, 0, (size_t)runs * sizeof(int32_t), s));

    std::vector<int32_t> flags((size_t)runs);
    const dim3 grid((unsigned)blocks, (unsigned)runs);
    for (int pass = 1; pass <= max_iter; ++pass) {
        hipLaunchKernelGGL(anchor_assign_kernel, grid, dim3(ANCH_THREADS), 0, s, wh, (long long)n, d_k, centroids, d_done, d_prev, d_sums, d_changed);
        MYOLO_CHECK_LAUNCH();
        hipLaunchKernelGGL(anchor_update_kernel, dim3((unsigned)runs), dim3(ANCH_KMAX), 0, s, d_k, centroids, d_done, d_sums, d_changed,
                           (long long*)counts, iterations, converged, max_iter);
        MYOLO_CHECK_LAUNCH();
        if (pass % ANCH_POLL == 0 && pass < max_iter) {
            ANCH_HIP(hipMemcpyAsync(flags.data(), d_done, (size_t)runs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            ANCH_HIP(hipStreamSynchronize(s));
            bool all = true;
            for (int r = 0; r < runs; ++r) all = all && flags[(size_t)r] != 0;
            if (all) break;
        }
    }
    hipLaunchKernelGGL(anchor_score_kernel, grid, dim3(ANCH_THREADS), 0, s, wh, (long long)n, d_k, centroids, d_prev, d_partial, assign);
    MYOLO_CHECK_LAUNCH();
    hipLaunchKernelGGL(anchor_finish_kernel, dim3((unsigned)runs), dim3(64), 0, s, d_partial, blocks, (long long)n, mean_iou);
    MYOLO_CHECK_LAUNCH();
    ANCH_HIP(hipStreamSynchronize(s));                          // run_k and the caller's outputs are final when this returns
#undef ANCH_HIP
    return MYOLO_OK;
}

}  // extern "C"
