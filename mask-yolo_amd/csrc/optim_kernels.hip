// The training recipe's optimiser pass (myolo/optim.py, Net.recipe_step; contract: include/myolo_hip_internal.h and DESIGN.md section 24):
// global-norm gradient clipping, AdamW's decoupled weight decay, the freeze mask and an EMA shadow of the weights in ONE read of p, g, m, v, behind
// a deterministic reduction of the gradient's squared norm.  Three launches per step, nothing returns to the host:
//     grad_sumsq_partials_kernel   per-thread double sums over the trainable groups, one double per workgroup (fixed tree in LDS)
//     grad_sumsq_finish_kernel     one workgroup: the partials in a fixed order, then the stats record (norm, scale, skipped, steps)
//     adamw_ema_kernel             the update; reads scale and the skip decision from the record
// The grids depend on n only and no atomics are used: sumsq has the same bits from run to run and on every rank that holds the same gradient.
//
// The update is restated operation for operation by tests/optim_ref.py, which is why this unit is compiled with -ffp-contract=off and asks for
// it again; sqrtf and the division are hipcc's default correctly rounded ones (no fast-math flag).
#include "myolo_common.h"
#include <math.h>
#pragma clang fp contract(off)

#define OPT_THREADS 256
#define OPT_UPDATE_BLOCKS 2048          // 256 CUs x 8 workgroups: the update and the swap grid-stride beyond this
static_assert((MYOLO_OPTIM_PARTIALS % OPT_THREADS) == 0, "the finish kernel walks the partials in whole rows of threads");

typedef float opt_f4 __attribute__((ext_vector_type(4)));

struct OptStats {
    double sumsq;
    float norm;
    float scale;
    int32_t skipped;
    int32_t steps;
};
static_assert(sizeof(OptStats) == 24, "the record's layout is part of the ABI");

// sum of the 256 per-thread values in a fixed order (valid in thread 0)
__device__ __forceinline__ double opt_block_sum(double x, double* red)
{
    red[threadIdx.x] = x;
    __syncthreads();
    for (int o = OPT_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_partials_kernel(const opt_f4* __restrict__ g, const uint8_t* __restrict__ flags,
                                                                          long long n4, float gs, double* __restrict__ partials)
{
    __shared__ double red[OPT_THREADS];
    const long long stride = (long long)gridDim.x * OPT_THREADS;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += stride) {
        if (!(flags[i] & 1)) continue;                       // a frozen group is not read: a non-finite value there does not skip the step
        const opt_f4 q = g[i];
        const float x0 = q.x * gs, x1 = q.y * gs, x2 = q.z * gs, x3 = q.w * gs;
        acc += (double)x0 * (double)x0;
        acc += (double)x1 * (double)x1;
        acc += (double)x2 * (double)x2;
        acc += (double)x3 * (double)x3;
    }
    const double s = opt_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_finish_kernel(const double* __restrict__ partials, int nparts, float clip,
                                                                        OptStats* __restrict__ stats)
{
    __shared__ double red[OPT_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += OPT_THREADS) acc += partials[i];
    const double s = opt_block_sum(acc, red);
    if (threadIdx.x == 0) {
        const bool finite = s - s == 0.0;                    // false for NaN and for either infinity
        float scale = 1.0f;
        if (!finite) scale = 0.0f;
        else if (clip != 0.0f && !(s <= (double)clip * (double)clip)) scale = (float)((double)clip / sqrt(s));
        stats->sumsq = s;
        stats->norm = (float)sqrt(s);
        stats->scale = scale;
        if (!finite) stats->skipped = stats->skipped + 1;
        stats->steps = stats->steps + 1;
    }
}

template <bool EMA>
__global__ __launch_bounds__(OPT_THREADS) void adamw_ema_kernel(opt_f4* __restrict__ p, const opt_f4* __restrict__ g, opt_f4* __restrict__ m,
                                                                opt_f4* __restrict__ v, opt_f4* __restrict__ ema,
                                                                const uint8_t* __restrict__ flags, long long n4,
                                                                const OptStats* __restrict__ stats, float lr_t, float b1, float b2, float eps,
                                                                float gs, float lr_wd, float ema_d, float ema_omd)
{
    const double sumsq = stats->sumsq;
    if (!(sumsq - sumsq == 0.0)) return;                     // a skipped step: nothing but stats changes (uniform over the whole grid)
    const float scale = stats->scale;
    const float omb1 = 1.f - b1, omb2 = 1.f - b2;
    const long long stride = (long long)gridDim.x * OPT_THREADS;
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += stride) {
        const unsigned f = flags[i];
        if (!(f & 1u)) continue;
        const opt_f4 p4 = p[i], g4 = g[i], m4 = m[i], v4 = v[i];
        opt_f4 e4 = {0.f, 0.f, 0.f, 0.f};
        if (EMA) e4 = ema[i];
        opt_f4 pn4, mn4, vn4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gi = (g4[k] * gs) * scale;
            const float mi = b1 * m4[k] + omb1 * gi;
            const float vi = b2 * v4[k] + (omb2 * gi) * gi;
            float pn = p4[k] - (lr_t * mi) / (sqrtf(vi) + eps);
            if (f & 2u) pn = pn - lr_wd * p4[k];
            if (EMA) e4[k] = ema_d * e4[k] + ema_omd * pn;
            mn4[k] = mi;
            vn4[k] = vi;
            pn4[k] = pn;
        }
        m[i] = mn4;
        v[i] = vn4;
        p[i] = pn4;
        if (EMA) ema[i] = e4;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void swap_f32_kernel(opt_f4* a, opt_f4* b, long long n4)
{
    const long long stride = (long long)gridDim.x * OPT_THREADS;
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += stride) {
        const opt_f4 x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

static inline unsigned opt_blocks(long long n4, long long cap)
{
    const long long b = (n4 + OPT_THREADS - 1) / OPT_THREADS;
    return (unsigned)(b < cap ? b : cap);
}

static inline bool opt_aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

extern "C" {

int myolo_grad_sumsq(const float* g, const uint8_t* flags, int64_t n, float gs, float clip, void* stats, double* partials, void* stream)
{
    MYOLO_REQUIRE(g && flags && stats && partials, "grad_sumsq: null pointer");
    MYOLO_REQUIRE(n > 0 && n % 4 == 0, "grad_sumsq: need n > 0 and n %% 4 == 0 (got n=%lld)", (long long)n);
    MYOLO_REQUIRE(clip >= 0.f && isfinite(clip), "grad_sumsq: clip must be finite and >= 0 (0 = off; got %g)", (double)clip);
    MYOLO_REQUIRE(opt_aligned16(g) && ((uintptr_t)stats & 7u) == 0 && ((uintptr_t)partials & 7u) == 0, "grad_sumsq: misaligned buffer");
    const long long n4 = n / 4;
    const unsigned nb = opt_blocks(n4, MYOLO_OPTIM_PARTIALS);
    hipLaunchKernelGGL(grad_sumsq_partials_kernel, dim3(nb), dim3(OPT_THREADS), 0, (hipStream_t)stream, (const opt_f4*)g, flags, n4, gs,
                       partials);
    MYOLO_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, (const double*)partials, (int)nb, clip,
                       (OptStats*)stats);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema_or_null, const uint8_t* flags, int64_t n, const void* stats,
                         float lr_t, float b1, float b2, float eps, float gs, float lr_wd, float ema_d, float ema_omd, void* stream)
{
    MYOLO_REQUIRE(p && g && m && v && flags && stats, "adamw_ema_step: null pointer");
    MYOLO_REQUIRE(n > 0 && n % 4 == 0, "adamw_ema_step: need n > 0 and n %% 4 == 0 (got n=%lld)", (long long)n);
    MYOLO_REQUIRE(opt_aligned16(p) && opt_aligned16(g) && opt_aligned16(m) && opt_aligned16(v) && opt_aligned16(ema_or_null) &&
                  ((uintptr_t)stats & 7u) == 0, "adamw_ema_step: misaligned buffer");
    const long long n4 = n / 4;
    const unsigned nb = opt_blocks(n4, OPT_UPDATE_BLOCKS);
    if (ema_or_null)
        hipLaunchKernelGGL(adamw_ema_kernel<true>, dim3(nb), dim3(OPT_THREADS), 0, (hipStream_t)stream, (opt_f4*)p, (const opt_f4*)g, (opt_f4*)m,
                           (opt_f4*)v, (opt_f4*)ema_or_null, flags, n4, (const OptStats*)stats, lr_t, b1, b2, eps, gs, lr_wd, ema_d, ema_omd);
    else
        hipLaunchKernelGGL(adamw_ema_kernel<false>, dim3(nb), dim3(OPT_THREADS), 0, (hipStream_t)stream, (opt_f4*)p, (const opt_f4*)g, (opt_f4*)m,
                           (opt_f4*)v, (opt_f4*)nullptr, flags, n4, (const OptStats*)stats, lr_t, b1, b2, eps, gs, lr_wd, ema_d, ema_omd);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_swap_f32(float* a, float* b, int64_t n, void* stream)
{
    MYOLO_REQUIRE(a && b, "swap_f32: null pointer");
    MYOLO_REQUIRE(n > 0 && n % 4 == 0, "swap_f32: need n > 0 and n %% 4 == 0 (got n=%lld)", (long long)n);
    MYOLO_REQUIRE(opt_aligned16(a) && opt_aligned16(b), "swap_f32: misaligned buffer");
    const long long n4 = n / 4;
    hipLaunchKernelGGL(swap_f32_kernel, dim3(opt_blocks(n4, OPT_UPDATE_BLOCKS)), dim3(OPT_THREADS), 0, (hipStream_t)stream, (opt_f4*)a,
                       (opt_f4*)b, n4);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

}  // extern "C"
