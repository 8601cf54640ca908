// Inference input of any size (MaskYOLO.detect / detect_many, engine.Net.resize_to_frame): a batch of uint8 [h,w,3] images of MIXED sizes, packed back
// to back in one buffer, is resized to the network frame [B,H,W,3] on the device -- myolo_utils.resize_image's arithmetic, so the result is the one the
// host function gives, bit for bit, without its padded float64 copy of the whole photograph.
//
// The arithmetic is a contract: per image and channel it is myolo_utils.resize(image, (H, W), preserve_range=True).astype(uint8),
// every operation below ONE IEEE binary64 operation in that function's order -- this unit is compiled with -ffp-contract=off and asks for it again
// here.  resize() clips its result to the value range of the WHOLE source image (all channels), so the call makes two launches: a per-image
// minimum / maximum over the source bytes, then the sampling pass.
#include "myolo_common.h"
#pragma clang fp contract(off)

#define RSZ_THREADS 256
#define RSZ_WAVES (RSZ_THREADS / 64)
#define RSZ_LOADS 8              // 16-byte loads a thread of the min/max kernel keeps in flight
#define RSZ_GRID_BLOCKS 2048     // min/max workgroups of a whole grid, all images (eight per CU: long-lived workgroups stream faster than many short ones)

typedef unsigned short rsz_us2 __attribute__((ext_vector_type(2)));

// two 16-bit lanes per word (v_pk_min_u16 / v_pk_max_u16): a word's even bytes in one operand, its odd bytes in the other
__device__ __forceinline__ uint32_t rsz_pk_min(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(rsz_us2, a), __builtin_bit_cast(rsz_us2, b)));
}
__device__ __forceinline__ uint32_t rsz_pk_max(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(rsz_us2, a), __builtin_bit_cast(rsz_us2, b)));
}
__device__ __forceinline__ void rsz_fold_word(uint32_t v, uint32_t& mn, uint32_t& mx)
{
    const uint32_t e = v & 0x00ff00ffu, o = (v >> 8) & 0x00ff00ffu;
    mn = rsz_pk_min(mn, rsz_pk_min(e, o));
    mx = rsz_pk_max(mx, rsz_pk_max(e, o));
}

// pass 1: mm[b], mm[B + b] = min, max over the 3*h*w bytes of image b.  An image starts at ANY byte of the packed buffer: the bytes in front of the first
// 16-byte boundary (head) and behind the last whole 16 (tail) are read one by one by workgroup 0, everything between as uint4.  Reduced in the wave
// (shuffles), across the waves in LDS, and one atomicMin / atomicMax per workgroup reaches memory; a workgroup with no byte of a (small) image leaves
// before any of that.  The caller set them to 255 and 0.
__global__ __launch_bounds__(RSZ_THREADS) void resize_minmax_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                    int* __restrict__ mm)
{
    __shared__ int red[RSZ_WAVES][2];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t off = desc[(int64_t)b * 3], h = desc[(int64_t)b * 3 + 1], w = desc[(int64_t)b * 3 + 2];
    const int64_t n = 3 * h * w;
    const uint8_t* p = src + off;
    int64_t head = (int64_t)((16 - ((uintptr_t)p & 15)) & 15);
    if (head > n) head = n;
    const int64_t nvec = (n - head) >> 4;
    const int64_t tail0 = head + (nvec << 4);
    const int64_t first = (int64_t)blockIdx.x * (RSZ_THREADS * RSZ_LOADS);
    if (blockIdx.x != 0 && first >= nvec) return;                // (uniform over the workgroup)
    uint32_t mn = 0x00ff00ffu, mx = 0u;
    const uint4* vp = (const uint4*)(p + head);
    const int64_t stride = (int64_t)gridDim.x * (RSZ_THREADS * RSZ_LOADS);
    for (int64_t i0 = first; i0 < nvec; i0 += stride) {
        uint4 v[RSZ_LOADS];
        const int64_t i = i0 + tid;
        if (i < nvec) {
#pragma unroll
            for (int j = 0; j < RSZ_LOADS; ++j) {                // (a load past the end re-reads this thread's first vector: harmless to min and max)
                const int64_t k = i + (int64_t)j * RSZ_THREADS;
                v[j] = vp[k < nvec ? k : i];
            }
#pragma unroll
            for (int j = 0; j < RSZ_LOADS; ++j) {
                rsz_fold_word(v[j].x, mn, mx);
                rsz_fold_word(v[j].y, mn, mx);
                rsz_fold_word(v[j].z, mn, mx);
                rsz_fold_word(v[j].w, mn, mx);
            }
        }
    }
    int lo = (int)min(mn & 0xffffu, mn >> 16), hi = (int)max(mx & 0xffffu, mx >> 16);
    if (blockIdx.x == 0) {                                       // head < 16 and tail < 16 bytes
        if (tid < head) { const int v = p[tid]; lo = min(lo, v); hi = max(hi, v); }
        if (tail0 + tid < n) { const int v = p[tail0 + tid]; lo = min(lo, v); hi = max(hi, v); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) { red[wave][0] = lo; red[wave][1] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < RSZ_WAVES; ++k) { lo = min(lo, red[k][0]); hi = max(hi, red[k][1]); }
        atomicMin(mm + b, lo);
        atomicMax(mm + gridDim.y + b, hi);
    }
}

// pass 2: one thread per output pixel, its three channels.  resize(): pixel centres aligned, taps floor / ceil of the source position, a tap outside the
// source reads 0, clipped to the source's range, truncated to a byte.
__global__ __launch_bounds__(RSZ_THREADS) void resize_sample_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                    const int* __restrict__ mm, uint8_t* __restrict__ out_u8,
                                                                    float* __restrict__ out_unit, int H, int W)
{
    const int b = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * RSZ_THREADS + threadIdx.x;
    if (pix >= HW) return;
    const int64_t off = desc[(int64_t)b * 3], h = desc[(int64_t)b * 3 + 1], w = desc[(int64_t)b * 3 + 2];
    const int64_t i = pix / W, j = pix - i * W;
    const double ys = ((double)i + .5) * ((double)h / (double)H) - .5;
    const double xs = ((double)j + .5) * ((double)w / (double)W) - .5;
    const double fy = floor(ys), fx = floor(xs);
    const double dy = ys - fy, dx = xs - fx;
    const int64_t y0 = (int64_t)fy, x0 = (int64_t)fx, y1 = (int64_t)ceil(ys), x1 = (int64_t)ceil(xs);       // -1 <= y0 <= y1 <= h (h, w >= 1)
    const bool in_y0 = y0 >= 0 && y0 < h, in_y1 = y1 >= 0 && y1 < h;
    const bool in_x0 = x0 >= 0 && x0 < w, in_x1 = x1 >= 0 && x1 < w;
    const uint8_t* p = src + off;
    const int64_t a00 = (y0 * w + x0) * 3, a01 = (y0 * w + x1) * 3, a10 = (y1 * w + x0) * 3, a11 = (y1 * w + x1) * 3;
    const double lo = (double)mm[b], hi = (double)mm[gridDim.y + b];
    const int64_t o = ((int64_t)b * HW + pix) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p00 = (in_y0 && in_x0) ? (double)p[a00 + c] : 0.0, p01 = (in_y0 && in_x1) ? (double)p[a01 + c] : 0.0;
        const double p10 = (in_y1 && in_x0) ? (double)p[a10 + c] : 0.0, p11 = (in_y1 && in_x1) ? (double)p[a11 + c] : 0.0;
        const double top = (1.0 - dx) * p00 + dx * p01;
        const double bot = (1.0 - dx) * p10 + dx * p11;
        double v = (1.0 - dy) * top + dy * bot;
        v = fmin(fmax(v, lo), hi);                               // np.clip(out, a.min(), a.max())
        const int u = (int)v;                                    // .astype(uint8) of a value in [0, 255]: truncation
        if (out_u8) out_u8[o + c] = (uint8_t)u;
        if (out_unit) out_unit[o + c] = (float)((double)u / 255.0);      // myolo_u8_to_unit_f32's quotient
    }
}

extern "C" {

size_t myolo_resize_images_ws_bytes(int B)
{
    if (B <= 0) return 0;
    return (size_t)B * 2 * sizeof(int);
}

int myolo_resize_images_u8(const uint8_t* src, size_t src_bytes, const int64_t* desc, const int64_t* desc_host, uint8_t* out_u8, float* out_unit,
                           int B, int H, int W, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(src && desc && desc_host, "resize_images: null pointer");
    MYOLO_REQUIRE(out_u8 || out_unit, "resize_images: null pointer (at least one of out_u8, out_unit is needed)");
    MYOLO_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffll - RSZ_THREADS,
                  "resize_images: bad sizes (B=%d, H=%d, W=%d)", B, H, W);
    const uint64_t cap = (uint64_t)src_bytes / 3;                // pixels the buffer can hold
    int64_t nmax = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t off = desc_host[b * 3], h = desc_host[b * 3 + 1], w = desc_host[b * 3 + 2];
        MYOLO_REQUIRE(h >= 1 && w >= 1, "resize_images: image %d has no pixels (h=%lld, w=%lld)", b, (long long)h, (long long)w);
        // 3*h*w <= src_bytes without forming a product that could overflow, then the offset
        MYOLO_REQUIRE(off >= 0 && (uint64_t)w <= cap && (uint64_t)h <= cap / (uint64_t)w && (uint64_t)off <= (uint64_t)src_bytes - (uint64_t)(3 * h * w),
                      "resize_images: image %d (offset %lld, %lld x %lld x 3) does not fit the %zu source bytes", b, (long long)off, (long long)h,
                      (long long)w, src_bytes);
        if (3 * h * w > nmax) nmax = 3 * h * w;
    }
    MYOLO_REQUIRE(ws && ws_bytes >= myolo_resize_images_ws_bytes(B), "resize_images: workspace too small (%zu needed, %zu given)",
                  myolo_resize_images_ws_bytes(B), ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    int* mm = (int*)ws;
    // mm = [B] minima, then [B] maxima, at their identities
    if (hipMemsetD32Async((hipDeviceptr_t)mm, 255, (size_t)B, s) != hipSuccess || hipMemsetAsync(mm + B, 0, (size_t)B * sizeof(int), s) != hipSuccess) {
        (void)hipGetLastError();
        MYOLO_REQUIRE(false, "resize_images: workspace fill failed");
    }
    const int64_t per = (int64_t)RSZ_THREADS * RSZ_LOADS * 16;   // bytes one workgroup reads per round
    // workgroups per image: what the largest image needs for one round each, cut to the grid's share in WHOLE rounds (no workgroup a round longer than the rest)
    int64_t gx = (nmax + per - 1) / per;
    const int64_t share = RSZ_GRID_BLOCKS / B > 0 ? RSZ_GRID_BLOCKS / B : 1;
    if (gx > share) {
        const int64_t rounds = (gx + share - 1) / share;
        gx = (gx + rounds - 1) / rounds;
    }
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(resize_minmax_kernel, dim3((unsigned)gx, B), dim3(RSZ_THREADS), 0, s, src, desc, mm);
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(resize_sample_kernel, dim3((unsigned)((HW + RSZ_THREADS - 1) / RSZ_THREADS), B), dim3(RSZ_THREADS), 0, s, src, desc,
                       (const int*)mm, out_u8, out_unit, H, W);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

}  // extern "C"
