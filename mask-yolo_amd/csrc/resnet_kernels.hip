// ResNet-50 backbone operators (Keras-2.2 keras_applications ResNet50 v1, cfg.BACKBONE = "resnet50"): the 7x7/s2 stem conv,
// ZeroPadding(1) + MaxPool 3x3/s2, the stride-2 row gather / scatter of the strided 1x1 convs and the residual join.  Every other layer
// of the network runs on the kernels the MobileNet path already uses (pointwise GEMMs, 3x3 convs, BatchNorm statistics / apply /
// backward).  Every kernel here is deterministic: no atomics, every sum in a fixed order.
#include "myolo_common.h"
#include "../../include/myolo_hip.h"

namespace {

constexpr int STEM_K = 7 * 7 * 3;      // 147 taps of conv1
constexpr int STEM_KP = 160;           // padded to a multiple of the GEMM's K step (16): the fast MFMA kernels take it

inline int blocks_for(long long n)
{
    long long b = (n + 255) / 256;
    if (b > 16384) b = 16384;
    if (b < 1) b = 1;
    return (int)b;
}

__device__ __forceinline__ float act_f(float v, int act)
{
    if (act == MYOLO_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == MYOLO_ACT_RELU6) return fminf(fmaxf(v, 0.f), 6.f);
    return v;
}

// col [M][STEM_KP]: row m = output pixel (n, oh, ow) of ZeroPadding2D(3) + Conv2D 7x7 stride 2 'valid'; column (kh*7 + kw)*3 + ci, the
// Keras HWIO kernel's row order; column 147 = 1 (it meets the bias, kept as row 147 of the padded weights), 148..159 = 0.  A workgroup fills
// STEM_ROWS whole rows (coalesced stores, 32-bit index arithmetic: M < 2^31 is checked by the callers)
constexpr int STEM_ROWS = 32;
__global__ __launch_bounds__(256) void stem_im2col_kernel(const float* __restrict__ x, float* __restrict__ col, int M, int H, int W, int Ho, int Wo)
{
    const int m0 = blockIdx.x * STEM_ROWS;
    for (int j = threadIdx.x; j < STEM_ROWS * STEM_KP; j += 256) {
        const int r = j / STEM_KP, k = j - r * STEM_KP;
        const int m = m0 + r;
        if (m >= M) break;
        float v = k == STEM_K ? 1.f : 0.f;
        if (k < STEM_K) {
            const int ow = m % Wo, t = m / Wo;
            const int oh = t % Ho, n = t / Ho;
            const int ci = k % 3, kw = (k / 3) % 7, kh = k / 21;
            const int ih = 2 * oh - 3 + kh, iw = 2 * ow - 3 + kw;
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = x[(((long long)n * H + ih) * W + iw) * 3 + ci];
        }
        col[(long long)m * STEM_KP + k] = v;
    }
}

// wp [STEM_KP][C]: rows 0..146 = w, row 147 = bias (0 without one), rows 148..159 = 0
__global__ void stem_pad_weight_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ wp, int C)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < STEM_KP * C; i += gridDim.x * blockDim.x) {
        const int r = i / C;
        wp[i] = r < STEM_K ? w[i] : (r == STEM_K && bias ? bias[i - STEM_K * C] : 0.f);
    }
}

// dw [147][C] and db [C] out of the padded weight gradient [STEM_KP][C] (row 147 = sum over rows of dy: the bias gradient)
__global__ void stem_unpad_grad_kernel(const float* __restrict__ dwp, float* __restrict__ dw, float* __restrict__ db, int C)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (STEM_K + 1) * C; i += gridDim.x * blockDim.x) {
        if (i < STEM_K * C) dw[i] = dwp[i];
        else if (db) db[i - STEM_K * C] = dwp[i];
    }
}

// ZeroPadding2D(1) + MaxPool2D 3x3 stride 2 'valid' on act(x*scale + shift) (scale == nullptr: on x).  One thread per output quad of
// channels; arg = window index 0..8 (row-major) of the FIRST maximum; a padding cell takes part with the value 0.
__global__ void maxpool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                   float* __restrict__ y, uint8_t* __restrict__ arg, int N, int H, int W, int C, int Ho, int Wo)
{
    const int C4 = C / 4;
    const long long total = (long long)N * Ho * Wo * C4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i % C4) * 4;
        const long long p = i / C4;
        const int ow = (int)(p % Wo);
        const long long t = p / Wo;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (scale) {
            sc = *reinterpret_cast<const float4*>(scale + c);
            sh = *reinterpret_cast<const float4*>(shift + c);
        }
        float best[4];
        int bk[4] = {0, 0, 0, 0};
        for (int k = 0; k < 9; ++k) {
            const int ih = 2 * oh - 1 + k / 3, iw = 2 * ow - 1 + k % 3;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
                const float4 q = *reinterpret_cast<const float4*>(x + (((long long)n * H + ih) * W + iw) * C + c);
                if (scale) {       // the multiply and the add rounded separately (no contraction): the same bits as BatchNorm's apply pass
                    v[0] = act_f(__fadd_rn(__fmul_rn(q.x, sc.x), sh.x), act);
                    v[1] = act_f(__fadd_rn(__fmul_rn(q.y, sc.y), sh.y), act);
                    v[2] = act_f(__fadd_rn(__fmul_rn(q.z, sc.z), sh.z), act);
                    v[3] = act_f(__fadd_rn(__fmul_rn(q.w, sc.w), sh.w), act);
                } else {
                    v[0] = act_f(q.x, act); v[1] = act_f(q.y, act); v[2] = act_f(q.z, act); v[3] = act_f(q.w, act);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k == 0 || v[j] > best[j]) { best[j] = v[j]; bk[j] = k; }
            }
        }
        *reinterpret_cast<float4*>(y + p * C + c) = make_float4(best[0], best[1], best[2], best[3]);
        *reinterpret_cast<uchar4*>(arg + p * C + c) = make_uchar4((uint8_t)bk[0], (uint8_t)bk[1], (uint8_t)bk[2], (uint8_t)bk[3]);
    }
}

// gradient wrt the pool's input (the activation): each input pixel gathers the gradients of the (at most four) windows that chose it,
// in window order (oh, then ow ascending).  A window that chose a padding cell contributes to no input.
__global__ void maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ arg, float* __restrict__ dx,
                                   int N, int H, int W, int C, int Ho, int Wo)
{
    const int C4 = C / 4;
    const long long total = (long long)N * H * W * C4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i % C4) * 4;
        const long long p = i / C4;
        const int w = (int)(p % W);
        const long long t = p / W;
        const int h = (int)(t % H);
        const int n = (int)(t / H);
        const int oh0 = h / 2, oh1 = min((h + 1) / 2, Ho - 1);
        const int ow0 = w / 2, ow1 = min((w + 1) / 2, Wo - 1);
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int oh = oh0; oh <= oh1; ++oh)
            for (int ow = ow0; ow <= ow1; ++ow) {
                const int k = (h - (2 * oh - 1)) * 3 + (w - (2 * ow - 1));
                const long long o = (((long long)n * Ho + oh) * Wo + ow) * C + c;
                const uchar4 a = *reinterpret_cast<const uchar4*>(arg + o);
                const float4 g = *reinterpret_cast<const float4*>(dy + o);
                if (a.x == k) s[0] += g.x;
                if (a.y == k) s[1] += g.y;
                if (a.z == k) s[2] += g.z;
                if (a.w == k) s[3] += g.w;
            }
        *reinterpret_cast<float4*>(dx + p * C + c) = make_float4(s[0], s[1], s[2], s[3]);
    }
}

// xs [N][Ho][Wo][C] = x [N][2i][2j][C]: the positions a Conv2D 1x1 stride 2 'valid' reads
__global__ void gather_s2_kernel(const float* __restrict__ x, float* __restrict__ xs, int N, int H, int W, int C, int Ho, int Wo)
{
    const int C4 = C / 4;
    const long long total = (long long)N * Ho * Wo * C4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i % C4) * 4;
        const long long p = i / C4;
        const int j = (int)(p % Wo);
        const long long t = p / Wo;
        const int r = (int)(t % Ho);
        const int n = (int)(t / Ho);
        *reinterpret_cast<float4*>(xs + p * C + c) =
            *reinterpret_cast<const float4*>(x + (((long long)n * H + 2 * r) * W + 2 * j) * C + c);
    }
}

// dx [N][H][W][C] = (a + b) at the even rows / columns, 0 elsewhere (b optional)
__global__ void scatter_s2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ dx, int N, int H, int W, int C,
                                  int Ho, int Wo)
{
    const int C4 = C / 4;
    const long long total = (long long)N * H * W * C4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i % C4) * 4;
        const long long p = i / C4;
        const int w = (int)(p % W);
        const long long t = p / W;
        const int h = (int)(t % H);
        const int n = (int)(t / H);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (((h | w) & 1) == 0) {
            const long long o = (((long long)n * Ho + h / 2) * Wo + w / 2) * C + c;
            v = *reinterpret_cast<const float4*>(a + o);
            if (b) {
                const float4 q = *reinterpret_cast<const float4*>(b + o);
                v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
            }
        }
        *reinterpret_cast<float4*>(dx + p * C + c) = v;
    }
}

// out = ReLU(y*s + t + r), r = sc*s1 + t1 (projection shortcut, s1 != nullptr) or sc (identity shortcut)
__global__ void residual_fwd_kernel(const float* __restrict__ y, const float* __restrict__ s, const float* __restrict__ t,
                                    const float* __restrict__ sc, const float* __restrict__ s1, const float* __restrict__ t1,
                                    float* __restrict__ out, long long nq, int C)
{
    const int C4 = C / 4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) {
        const int c = (int)(i % C4) * 4;
        const float4 a = reinterpret_cast<const float4*>(y)[i];
        const float4 r = reinterpret_cast<const float4*>(sc)[i];
        const float4 ks = *reinterpret_cast<const float4*>(s + c), kt = *reinterpret_cast<const float4*>(t + c);
        float4 q;
        q.x = fmaf(a.x, ks.x, kt.x); q.y = fmaf(a.y, ks.y, kt.y); q.z = fmaf(a.z, ks.z, kt.z); q.w = fmaf(a.w, ks.w, kt.w);
        if (s1) {
            const float4 ps = *reinterpret_cast<const float4*>(s1 + c), pt = *reinterpret_cast<const float4*>(t1 + c);
            q.x += fmaf(r.x, ps.x, pt.x); q.y += fmaf(r.y, ps.y, pt.y); q.z += fmaf(r.z, ps.z, pt.z); q.w += fmaf(r.w, ps.w, pt.w);
        } else {
            q.x += r.x; q.y += r.y; q.z += r.z; q.w += r.w;
        }
        reinterpret_cast<float4*>(out)[i] = make_float4(fmaxf(q.x, 0.f), fmaxf(q.y, 0.f), fmaxf(q.z, 0.f), fmaxf(q.w, 0.f));
    }
}

// g = dout * [out > 0]
__global__ void residual_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, float* __restrict__ g, long long nq)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) {
        const float4 d = reinterpret_cast<const float4*>(dout)[i];
        const float4 o = reinterpret_cast<const float4*>(out)[i];
        reinterpret_cast<float4*>(g)[i] = make_float4(o.x > 0.f ? d.x : 0.f, o.y > 0.f ? d.y : 0.f, o.z > 0.f ? d.z : 0.f, o.w > 0.f ? d.w : 0.f);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// output rows / columns of ZeroPadding(1) + 3x3/s2 'valid', of ZeroPadding(3) + 7x7/s2 'valid' and of 1x1/s2 'valid' alike
inline int s2_out(int h) { return (h - 1) / 2 + 1; }

}  // namespace

extern "C" {

size_t myolo_conv7x7s2_c3_ws_bytes(int N, int H, int W, int Cout)
{
    const long long M = (long long)N * s2_out(H) * s2_out(W);
    const size_t g = myolo_workspace_bytes(M, STEM_KP, Cout), b = myolo_pwconv1x1_bnstats_ws_bytes(M, STEM_KP, Cout);
    return align256((size_t)M * STEM_KP * sizeof(float)) + align256((size_t)STEM_KP * Cout * sizeof(float)) + (g > b ? g : b);
}

// im2col of the images and the padded weights (bias in row 147) into ws; returns the rest of ws for the GEMM behind them
static int stem_prepare(const char* who, const float* x, const float* w, const float* bias, int N, int H, int W, int Cout, void* ws, size_t ws_bytes,
                        hipStream_t s, float** col, float** wp, long long* M, void** rest, size_t* rest_bytes)
{
    MYOLO_REQUIRE(x && N > 0 && H > 0 && W > 0 && Cout > 0 && (Cout & 3) == 0, "%s: bad arguments", who);
    *M = (long long)N * s2_out(H) * s2_out(W);
    MYOLO_REQUIRE(*M <= 0x7fffffffLL, "%s: %lld output pixels, more than 2^31 - 1", who, *M);
    const size_t cb = align256((size_t)*M * STEM_KP * sizeof(float)), wb = align256((size_t)STEM_KP * Cout * sizeof(float));
    if (cb + wb > ws_bytes || !ws) {
        myolo_set_error("%s: workspace too small (%zu needed, %zu given)", who, cb + wb, ws_bytes);
        return MYOLO_EWORKSPACE;
    }
    *col = (float*)ws;
    *wp = (float*)((char*)ws + cb);
    *rest = (char*)ws + cb + wb;
    *rest_bytes = ws_bytes - cb - wb;
    hipLaunchKernelGGL(stem_im2col_kernel, dim3((unsigned)cdiv64(*M, STEM_ROWS)), dim3(256), 0, s, x, *col, (int)*M, H, W, s2_out(H), s2_out(W));
    if (w) hipLaunchKernelGGL(stem_pad_weight_kernel, dim3(blocks_for((long long)STEM_KP * Cout)), dim3(256), 0, s, w, bias, *wp, Cout);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_conv7x7s2_c3_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cout,
                           void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(w && y, "conv7x7s2_c3_fwd: bad arguments");
    float *col, *wp;
    long long M;
    void* rest;
    size_t rb;
    const int rc = stem_prepare("conv7x7s2_c3_fwd", x, w, bias, N, H, W, Cout, ws, ws_bytes, (hipStream_t)stream, &col, &wp, &M, &rest, &rb);
    if (rc) return rc;
    // [M][160] x [160][Cout] on the pointwise MFMA path (fp32 products formed as cfg.FP32_MATMUL asks); the bias comes in through column 147
    return myolo_pwconv1x1_fwd(col, wp, nullptr, y, M, STEM_KP, Cout, rest, rb, stream);
}

int myolo_conv7x7s2_c3_bnstats_fwd(const float* x, const float* w, const float* bias, float* y, const float* gamma, const float* beta, float* mean,
                                   float* var, float* scale, float* shift, float* moving_mean, float* moving_var, int N, int H, int W, int Cout,
                                   void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(w && y && myolo_pwconv1x1_bnstats_ok(STEM_KP, Cout), "conv7x7s2_c3_bnstats_fwd: bad arguments");
    float *col, *wp;
    long long M;
    void* rest;
    size_t rb;
    const int rc = stem_prepare("conv7x7s2_c3_bnstats_fwd", x, w, bias, N, H, W, Cout, ws, ws_bytes, (hipStream_t)stream, &col, &wp, &M, &rest, &rb);
    if (rc) return rc;
    // the GEMM leaves per-tile column sums of y (the bias included: it enters the moving mean) and the finish forms the batch statistics
    return myolo_pwconv1x1_bnstats_fwd(col, nullptr, nullptr, MYOLO_ACT_NONE, wp, y, gamma, beta, mean, var, scale, shift, moving_mean, moving_var,
                                       M, STEM_KP, Cout, 3, rest, rb, stream);
}

int myolo_conv7x7s2_c3_affine_act_fwd(const float* x, const float* w, const float* bias, const float* scale, const float* shift, int act, float* y,
                                      int N, int H, int W, int Cout, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(w && y && scale && shift, "conv7x7s2_c3_affine_act_fwd: bad arguments");
    float *col, *wp;
    long long M;
    void* rest;
    size_t rb;
    const int rc = stem_prepare("conv7x7s2_c3_affine_act_fwd", x, w, bias, N, H, W, Cout, ws, ws_bytes, (hipStream_t)stream, &col, &wp, &M, &rest, &rb);
    if (rc) return rc;
    return myolo_pwconv1x1_affine_act_fwd(col, wp, scale, shift, act, y, M, STEM_KP, Cout, rest, rb, stream);
}

int myolo_conv7x7s2_c3_bwd_weight(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cout,
                                  void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(dy && dw && al16(dy), "conv7x7s2_c3_bwd_weight: bad arguments");
    float *col, *dwp;
    long long M;
    void* rest;
    size_t rb;
    hipStream_t s = (hipStream_t)stream;
    int rc = stem_prepare("conv7x7s2_c3_bwd_weight", x, nullptr, nullptr, N, H, W, Cout, ws, ws_bytes, s, &col, &dwp, &M, &rest, &rb);
    if (rc) return rc;
    // dW [160][Cout] = col^T dy: the pointwise weight gradient (per-workgroup partials, fixed-order reduction); row 147 is the bias gradient
    rc = myolo_pwconv1x1_bwd_weight(col, dy, dwp, M, STEM_KP, Cout, rest, rb, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(stem_unpad_grad_kernel, dim3(blocks_for((long long)(STEM_K + 1) * Cout)), dim3(256), 0, s, dwp, dw, db, Cout);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_maxpool3x3s2_fwd(const float* x, const float* scale, const float* shift, int act, float* y, uint8_t* arg,
                           int N, int H, int W, int C, void* stream)
{
    MYOLO_REQUIRE(x && y && arg && N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && (!scale) == (!shift) && al16(x) && al16(y) &&
                  ((uintptr_t)arg & 3) == 0 && (!scale || (al16(scale) && al16(shift))), "maxpool3x3s2_fwd: bad arguments");
    const int Ho = s2_out(H), Wo = s2_out(W);
    const long long n = (long long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, x, scale, shift, act, y, arg, N, H, W, C, Ho, Wo);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_maxpool3x3s2_bwd(const float* dy, const uint8_t* arg, float* dx, int N, int H, int W, int C, void* stream)
{
    MYOLO_REQUIRE(dy && arg && dx && N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && al16(dy) && al16(dx) && ((uintptr_t)arg & 3) == 0,
                  "maxpool3x3s2_bwd: bad arguments");
    const int Ho = s2_out(H), Wo = s2_out(W);
    const long long n = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, dy, arg, dx, N, H, W, C, Ho, Wo);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_gather_s2(const float* x, float* xs, int N, int H, int W, int C, void* stream)
{
    MYOLO_REQUIRE(x && xs && N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && al16(x) && al16(xs), "gather_s2: bad arguments");
    const int Ho = s2_out(H), Wo = s2_out(W);
    const long long n = (long long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(gather_s2_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, x, xs, N, H, W, C, Ho, Wo);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_scatter_s2(const float* a, const float* b, float* dx, int N, int H, int W, int C, void* stream)
{
    MYOLO_REQUIRE(a && dx && N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && al16(a) && al16(dx) && (!b || al16(b)), "scatter_s2: bad arguments");
    const int Ho = s2_out(H), Wo = s2_out(W);
    const long long n = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(scatter_s2_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, a, b, dx, N, H, W, C, Ho, Wo);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_residual_fwd(const float* y, const float* scale, const float* shift, const float* sc, const float* sc_scale, const float* sc_shift,
                       float* out, int64_t M, int C, void* stream)
{
    MYOLO_REQUIRE(y && scale && shift && sc && out && M > 0 && C > 0 && (C & 3) == 0 && (!sc_scale) == (!sc_shift) && al16(y) && al16(sc) &&
                  al16(out) && al16(scale) && al16(shift) && (!sc_scale || (al16(sc_scale) && al16(sc_shift))), "residual_fwd: bad arguments");
    const long long nq = (long long)M * C / 4;
    hipLaunchKernelGGL(residual_fwd_kernel, dim3(blocks_for(nq)), dim3(256), 0, (hipStream_t)stream, y, scale, shift, sc, sc_scale, sc_shift,
                       out, nq, C);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_residual_bwd(const float* dout, const float* out, float* g, int64_t n, void* stream)
{
    MYOLO_REQUIRE(dout && out && g && n > 0 && (n & 3) == 0 && al16(dout) && al16(out) && al16(g), "residual_bwd: bad arguments");
    hipLaunchKernelGGL(residual_bwd_kernel, dim3(blocks_for(n / 4)), dim3(256), 0, (hipStream_t)stream, dout, out, g, (long long)(n / 4));
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

}  // extern "C"
