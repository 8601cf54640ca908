// Photometric augmentation on the device (myolo/augment.py: Photometric): the last stage of the device augmenter, on the float image the stage
// before it wrote.  Per image one row of 32 doubles -- a 3x4 colour transform, a noise deviation and key, a blur radius and its 16 weights --
// and per pixel: separable Gaussian blur with reflected borders, the colour transform, hashed noise, a clamp to [0, 1].
//
// The arithmetic is a contract ("Photometric augmentation"): every operation below is ONE IEEE binary64 operation in the order
// written -- this unit is compiled with -ffp-contract=off and asks for it again here -- so a numpy restatement (tests/photometric_ref.py)
// reproduces every output bit.  No atomics and no hand-off between workgroups: two calls give the same bytes.
#include "myolo_common.h"
#pragma clang fp contract(off)

#define PHO_THREADS 256
#define PHO_ROW 32           // doubles per image row
#define PHO_MAXR 15          // largest blur radius: the row holds w_0 .. w_15

// reflect-101: ... 2 1 | 0 1 2 .. n-1 | n-2 n-3 ...; valid however far i lies outside (a radius beyond the side wraps several times)
__device__ __forceinline__ int pho_refl(int i, int n)
{
    if (i >= 0 && i < n) return i;
    if (n == 1) return 0;
    const int P = 2 * (n - 1);
    const int m = ((i % P) + P) % P;
    return m < n ? m : P - m;
}

// the row's radius under the caller's bound; anything that is not a number >= 1 (NaN included) gives 0 before the conversion
__device__ __forceinline__ int pho_radius(const double* __restrict__ row, int max_radius)
{
    const double rd = row[14];
    if (!(rd >= 1.0)) return 0;
    return rd < (double)max_radius ? (int)rd : max_radius;
}

// pass 1 of the blur: one thread per float of the image (pixel, channel); h goes to the workspace as a double, never rounded to float
__global__ __launch_bounds__(PHO_THREADS) void photometric_blur_rows_kernel(const float* __restrict__ src, const double* __restrict__ rows,
                                                                            double* __restrict__ hbuf, int max_radius, int H, int W)
{
    const int b = blockIdx.y;
    const long long n = (long long)H * W * 3;
    const long long e = (long long)blockIdx.x * PHO_THREADS + threadIdx.x;
    if (e >= n) return;
    const double* __restrict__ row = rows + (size_t)b * PHO_ROW;
    const int r = pho_radius(row, max_radius);
    const long long pix = e / 3;
    const int c = (int)(e - pix * 3);
    const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
    const float* __restrict__ line = src + ((size_t)b * H + y) * (size_t)W * 3 + c;
    double h = row[16] * (double)line[(size_t)x * 3];
    for (int k = 1; k <= r; ++k) {
        const double lo = (double)line[(size_t)pho_refl(x - k, W) * 3], hi = (double)line[(size_t)pho_refl(x + k, W) * 3];
        h = h + row[16 + k] * (lo + hi);
    }
    hbuf[(size_t)b * n + e] = h;
}

__device__ __forceinline__ uint64_t pho_splitmix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// pass 2 (the only pass with max_radius = 0): a workgroup owns PHO_THREADS consecutive pixels.  BLUR: the vertical taps of the three h of a
// pixel are 24 contiguous bytes per thread and neighbours across the wave; without it h = w0 * s, as the first pass would have written it.
// Then the colour transform, the noise and the clamp; the floats pass through LDS and leave as contiguous runs.
template <bool BLUR>
__global__ __launch_bounds__(PHO_THREADS) void photometric_point_kernel(const float* __restrict__ src, const double* __restrict__ hbuf,
                                                                       const double* __restrict__ rows, float* __restrict__ images,
                                                                       int max_radius, int H, int W)
{
    __shared__ float s_img[PHO_THREADS * 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long HW = (long long)H * W;
    const long long pix0 = (long long)blockIdx.x * PHO_THREADS, pix = pix0 + tid;
    const int nv = (int)((HW - pix0) < PHO_THREADS ? (HW - pix0) : PHO_THREADS);      // pixels of this workgroup inside the image
    const double* __restrict__ row = rows + (size_t)b * PHO_ROW;
    if (tid < nv) {
        const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
        const double w0 = row[16];
        double v[3];
        if (BLUR) {
            const int r = pho_radius(row, max_radius);
            const double* __restrict__ col = hbuf + ((size_t)b * HW + x) * 3;
            const double* p = col + (size_t)y * W * 3;
            v[0] = w0 * p[0]; v[1] = w0 * p[1]; v[2] = w0 * p[2];
            for (int k = 1; k <= r; ++k) {
                const double* lo = col + (size_t)pho_refl(y - k, H) * W * 3;
                const double* hi = col + (size_t)pho_refl(y + k, H) * W * 3;
                const double wk = row[16 + k];
                v[0] = v[0] + wk * (lo[0] + hi[0]);
                v[1] = v[1] + wk * (lo[1] + hi[1]);
                v[2] = v[2] + wk * (lo[2] + hi[2]);
            }
        } else {
            const float* p = src + ((size_t)b * HW + pix) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double h = w0 * (double)p[c];
                v[c] = w0 * h;
            }
        }
        const double sd = row[12], kd = row[13];
        const uint64_t key = (kd >= 0.0 && kd < 4294967296.0) ? (uint64_t)kd : 0ull;      // (checked on the host; never an undefined conversion)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double u = ((row[c * 4] * v[0] + row[c * 4 + 1] * v[1]) + row[c * 4 + 2] * v[2]) + row[c * 4 + 3];
            const uint64_t j = (uint64_t)pix * 3 + c;
            const uint64_t z = pho_splitmix64((key << 32) | j);
            const uint32_t S = (uint32_t)(z & 0xffff) + (uint32_t)((z >> 16) & 0xffff) + (uint32_t)((z >> 32) & 0xffff) + (uint32_t)(z >> 48);
            const double nz = ((double)S - 131070.0) * (1.7320508075688772 / 65536.0);
            u = u + sd * nz;
            u = u > 0.0 ? u : 0.0;
            u = u < 1.0 ? u : 1.0;
            s_img[tid * 3 + c] = (float)u;
        }
    }
    __syncthreads();
    float* __restrict__ out = images + ((size_t)b * HW + pix0) * 3;
    for (int i = tid; i < nv * 3; i += PHO_THREADS) out[i] = s_img[i];
}

// [p, p + n) and [q, q + m) share a byte
static bool pho_overlap(const void* p, size_t n, const void* q, size_t m)
{
    const uintptr_t a = (uintptr_t)p, c = (uintptr_t)q;
    return p && q && n && m && a < c + m && c < a + n;
}

extern "C" {

size_t myolo_photometric_batch_ws_bytes(int B, int H, int W, int max_radius)
{
    if (B <= 0 || H <= 0 || W <= 0 || max_radius <= 0) return 0;
    return (size_t)B * H * W * 3 * sizeof(double);
}

int myolo_photometric_batch(const float* src_images, const double* rows, float* images, int max_radius, int B, int H, int W, void* ws,
                            size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(src_images && rows && images, "photometric_batch: null pointer");
    MYOLO_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W * 3 < (1ll << 31) - PHO_THREADS,
                  "photometric_batch: bad sizes (B=%d, H=%d, W=%d)", B, H, W);
    MYOLO_REQUIRE(max_radius >= 0 && max_radius <= PHO_MAXR, "photometric_batch: need 0 <= max_radius <= %d (got %d)", PHO_MAXR, max_radius);
    const long long HW = (long long)H * W;
    const size_t img_bytes = (size_t)B * HW * 3 * sizeof(float), need = myolo_photometric_batch_ws_bytes(B, H, W, max_radius);
    // the blur reads neighbours of a pixel while other workgroups write: the output may not lie over the input (nor over the rows)
    MYOLO_REQUIRE(!pho_overlap(src_images, img_bytes, images, img_bytes), "photometric_batch: the output lies over the input");
    MYOLO_REQUIRE(!pho_overlap(rows, (size_t)B * PHO_ROW * sizeof(double), images, img_bytes), "photometric_batch: the output lies over the rows");
    MYOLO_REQUIRE(need == 0 || (ws && ws_bytes >= need), "photometric_batch: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
    MYOLO_REQUIRE(need == 0 || (!pho_overlap(ws, need, images, img_bytes) && !pho_overlap(ws, need, src_images, img_bytes) &&
                                !pho_overlap(ws, need, rows, (size_t)B * PHO_ROW * sizeof(double))),
                  "photometric_batch: the workspace lies over an array");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((HW + PHO_THREADS - 1) / PHO_THREADS), B);
    if (max_radius > 0) {
        const dim3 grid3((unsigned)((HW * 3 + PHO_THREADS - 1) / PHO_THREADS), B);
        hipLaunchKernelGGL(photometric_blur_rows_kernel, grid3, dim3(PHO_THREADS), 0, s, src_images, rows, (double*)ws, max_radius, H, W);
        hipLaunchKernelGGL(photometric_point_kernel<true>, grid, dim3(PHO_THREADS), 0, s, src_images, (const double*)ws, rows, images, max_radius,
                           H, W);
    } else {
        hipLaunchKernelGGL(photometric_point_kernel<false>, grid, dim3(PHO_THREADS), 0, s, src_images, (const double*)nullptr, rows, images, 0,
                           H, W);
    }
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

}  // extern "C"
