// On-device training augmentation (myolo/augment.py: DeviceAugmenter): one more producer of the six training inputs, beside the Shapes
// producer of exact_kernels.hip.  It takes the resident bytes and instance masks of a batch plus one inverse affine map, gain and bias per
// image, and writes the warped image (bilinear), the warped instance masks (nearest) with empty instances dropped and the survivors compacted,
// their tight boxes (extract_bboxes) and BatchGenerator._encode's YOLO targets of those boxes.
// myolo_mosaic_batch (below the three passes it extends) does the same with four tiles per output image, each read from an image of the batch.
// myolo_copy_paste_batch is a second stage behind either: it pastes instances of one augmented image of the batch into another.
//
// The arithmetic is a contract ("On-device augmentation"): every operation below is ONE IEEE binary64 operation in the order
// written -- this unit is compiled with -ffp-contract=off and asks for it again here -- so a numpy restatement reproduces every output bit.
#include "myolo_common.h"
#pragma clang fp contract(off)

#define AUG_MAXT 32          // instance slots: bounds the LDS arrays of the stats and render kernels
#define AUG_THREADS 256
#define AUG_WAVES (AUG_THREADS / 64)

// stats[b][t] = {count, W - minx, maxx + 1, H - miny, maxy + 1}: a sum and four maxima, so that all-zero is the empty state (one memset)
#define AUG_STAT_INTS 5

__device__ __forceinline__ void aug_source(const double* __restrict__ p, int x, int y, double& sx, double& sy)
{
    sx = (p[0] * x + p[1] * y) + p[2];
    sy = (p[3] * x + p[4] * y) + p[5];
}

// nearest source pixel of the masks: floor(s + 0.5) inside the frame, or false
__device__ __forceinline__ bool aug_nearest(double sx, double sy, int H, int W, int& ix, int& iy)
{
    const double fx = floor(sx + 0.5), fy = floor(sy + 0.5);
    if (!(fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H)) return false;      // (also refuses NaN before the conversion)
    ix = (int)fx; iy = (int)fy;
    return true;
}

__device__ __forceinline__ int aug_wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// the T mask bytes of a pixel start at a multiple of T: when T and the base pointer are multiples of V they are read V bytes at a time
template <int V> __device__ __forceinline__ uint32_t aug_load(const uint8_t* p)
{
    if (V == 4) return *(const uint32_t*)p;
    if (V == 2) return *(const uint16_t*)p;
    return *p;
}

#define AUG_SPT 4            // output pixels per thread of the stats kernel

// pass 1: per (image, source instance) warped pixel count and extent.  A thread takes AUG_SPT output pixels (AUG_THREADS apart, so a wave's loads stay
// neighbours); count / extent are reduced across the wave (ballot + popcount, shuffles), then across the workgroup in LDS, and reach memory as at
// most one set of integer atomics per (workgroup, instance) -- none for an instance the workgroup did not see.
template <int V>
__global__ __launch_bounds__(AUG_THREADS) void augment_stats_kernel(const uint8_t* __restrict__ src_masks, const int32_t* __restrict__ src_ids,
                                                                    const double* __restrict__ params, int* __restrict__ stats,
                                                                    int H, int W, int T)
{
    __shared__ int red[AUG_WAVES][AUG_MAXT][AUG_STAT_INTS];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long HW = (long long)H * W;
    const uint8_t* mb = src_masks + (long long)b * HW * T;
    int px[AUG_SPT], py[AUG_SPT];
    long long off[AUG_SPT];                                    // byte offset of the source pixel's slots, or -1: no source pixel
#pragma unroll
    for (int j = 0; j < AUG_SPT; ++j) {
        const long long pix = ((long long)blockIdx.x * AUG_SPT + j) * AUG_THREADS + tid;
        py[j] = (int)(pix / W); px[j] = (int)(pix - (long long)py[j] * W);
        off[j] = -1;
        if (pix < HW) {                                        // (the ragged last workgroup keeps its lanes for the wave reductions)
            double sx, sy;
            int ix, iy;
            aug_source(params + (long long)b * 8, px[j], py[j], sx, sy);
            if (aug_nearest(sx, sy, H, W, ix, iy)) off[j] = ((long long)iy * W + ix) * T;
        }
    }
    for (int w = 0; w < T; w += V) {
        uint32_t word[AUG_SPT];
#pragma unroll
        for (int j = 0; j < AUG_SPT; ++j) word[j] = off[j] >= 0 ? aug_load<V>(mb + off[j] + w) : 0u;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int t = w + k;
            const bool live = src_ids[b * T + t] != 0;
            int cnt = 0, a = 0, c = 0, d = 0, e = 0;
#pragma unroll
            for (int j = 0; j < AUG_SPT; ++j) {
                const bool in = live && ((word[j] >> (8 * k)) & 0xffu) != 0;
                cnt += __popcll(__ballot(in));
                if (in) { a = max(a, W - px[j]); c = max(c, px[j] + 1); d = max(d, H - py[j]); e = max(e, py[j] + 1); }
            }
            if (cnt) {                                         // wave-uniform: it comes from ballots
                a = aug_wave_max(a); c = aug_wave_max(c); d = aug_wave_max(d); e = aug_wave_max(e);
            }
            if (lane == 0) { int* r = red[wave][t]; r[0] = cnt; r[1] = a; r[2] = c; r[3] = d; r[4] = e; }
        }
    }
    __syncthreads();
    if (tid < T) {
        int cnt = 0, v[4] = {0, 0, 0, 0};
        for (int w = 0; w < AUG_WAVES; ++w) {
            cnt += red[w][tid][0];
            for (int k = 0; k < 4; ++k) v[k] = max(v[k], red[w][tid][1 + k]);
        }
        if (cnt) {
            int* st = stats + ((long long)b * T + tid) * AUG_STAT_INTS;
            atomicAdd(st, cnt);
            for (int k = 0; k < 4; ++k) atomicMax(st + 1 + k, v[k]);
        }
    }
}

// BatchGenerator._encode's targets of ONE box -- the arithmetic of shapes_encode_kernel (exact_kernels.hip), in double: first-maximum anchor, a later
// box overwrites a shared cell, true_boxes wraps modulo T (tbi: the image's running true_boxes index).
__device__ __forceinline__ void aug_encode_target(int b, int cls, int x1, int y1, int x2, int y2, double cell_w, double cell_h,
                                                  const double* __restrict__ anchors, float* __restrict__ y_true, float* __restrict__ true_boxes,
                                                  int& tbi, int T, int G, int A, int C)
{
    const double cx = .5 * (x1 + x2) / cell_w, cy = .5 * (y1 + y2) / cell_h;
    const int gx = (int)floor(cx), gy = (int)floor(cy);
    if (gx < G && gy < G) {
        const double bw = (x2 - x1) / cell_w, bh = (y2 - y1) / cell_h;
        int best = 0;
        double max_iou = -1;
        for (int j = 0; j < A; ++j) {
            const double aw = anchors[2 * j], ah = anchors[2 * j + 1];
            const double iw = fmin(bw, aw), ih = fmin(bh, ah);
            const double inter = iw * ih;
            const double iou = inter / (bw * bh + aw * ah - inter);
            if (max_iou < iou) { best = j; max_iou = iou; }
        }
        float* yt = y_true + ((((long long)b * G + gy) * G + gx) * A + best) * (5 + C);
        yt[0] = (float)cx; yt[1] = (float)cy; yt[2] = (float)bw; yt[3] = (float)bh; yt[4] = 1.0f;
        if ((unsigned)cls < (unsigned)C) yt[5 + cls] = 1.0f;
        float* tb = true_boxes + ((long long)b * T + tbi) * 4;
        tb[0] = (float)cx; tb[1] = (float)cy; tb[2] = (float)bw; tb[3] = (float)bh;
        tbi = (tbi + 1) % T;
    }
}

// pass 2 (one workgroup per image): compaction of the surviving instances (load_image_gt's np.sum(mask) > 0 filter), boxes, class ids and
// BatchGenerator._encode's targets (aug_encode_target).  The outputs were zeroed by the caller.
__global__ void augment_encode_kernel(const int32_t* __restrict__ src_ids, const int* __restrict__ stats, int* __restrict__ slotmap,
                                      int32_t* __restrict__ gt_ids, int32_t* __restrict__ gt_boxes, float* __restrict__ y_true,
                                      float* __restrict__ true_boxes, const double* __restrict__ anchors, int H, int W, int T, int G, int A, int C)
{
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const double cell_w = (double)W / G, cell_h = (double)H / G;
    int m = 0, tbi = 0;
    for (int k = 0; k < T; ++k) {
        const int* st = stats + ((long long)b * T + k) * AUG_STAT_INTS;
        const int cls = src_ids[b * T + k];
        if (cls == 0 || st[0] <= 0) { slotmap[b * T + k] = -1; continue; }
        slotmap[b * T + k] = m;
        const int x1 = W - st[1], x2 = st[2], y1 = H - st[3], y2 = st[4];     // extract_bboxes: x2, y2 exclusive
        gt_ids[b * T + m] = cls;
        int32_t* gb = gt_boxes + ((long long)b * T + m) * 4;
        gb[0] = x1; gb[1] = y1; gb[2] = x2; gb[3] = y2;
        if (y_true) aug_encode_target(b, cls, x1, y1, x2, y2, cell_w, cell_h, anchors, y_true, true_boxes, tbi, T, G, A, C);
        ++m;
    }
}

// image: bilinear, a tap outside the frame reads cval; then gain, bias, clamp and the byte -> unit scale.  ib: the source image, out: 3 floats
__device__ __forceinline__ void aug_bilinear(const uint8_t* __restrict__ ib, double sx, double sy, const double* __restrict__ p, double cval,
                                             int H, int W, float* out)
{
    const double flx = floor(sx), fly = floor(sy);
    const double fx = sx - flx, fy = sy - fly;
    const bool near_x = flx >= -1.0 && flx < (double)W, near_y = fly >= -1.0 && fly < (double)H;       // some tap may be inside
    const int x0 = near_x ? (int)flx : -2, y0 = near_y ? (int)fly : -2;
    const bool in_x0 = x0 >= 0 && x0 < W, in_x1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool in_y0 = y0 >= 0 && y0 < H, in_y1 = y0 + 1 >= 0 && y0 + 1 < H;
    const uint8_t* r0 = ib + ((long long)y0 * W + x0) * 3;
    const uint8_t* r1 = r0 + (long long)W * 3;
    for (int c = 0; c < 3; ++c) {
        const double p00 = (in_y0 && in_x0) ? (double)r0[c] : cval, p01 = (in_y0 && in_x1) ? (double)r0[3 + c] : cval;
        const double p10 = (in_y1 && in_x0) ? (double)r1[c] : cval, p11 = (in_y1 && in_x1) ? (double)r1[3 + c] : cval;
        const double top = (1.0 - fx) * p00 + fx * p01;
        const double bot = (1.0 - fx) * p10 + fx * p11;
        double v = (1.0 - fy) * top + fy * bot;
        v = fmin(fmax(p[6] * v + p[7], 0.0), 255.0);
        out[c] = (float)(v / 255.0);
    }
}

// the end of a render workgroup: its nv pixels' floats and mask bytes leave LDS as contiguous runs (consecutive lanes, consecutive words)
__device__ __forceinline__ void aug_write_runs(const float* s_img, const uint8_t* s_msk, float* __restrict__ images, uint8_t* __restrict__ masks,
                                               int b, long long HW, long long pix0, int nv, int T, int words_ok, int tid)
{
    float* ip = images + ((long long)b * HW + pix0) * 3;
    for (int i = tid; i < nv * 3; i += AUG_THREADS) ip[i] = s_img[i];
    uint8_t* mo = masks + ((long long)b * HW + pix0) * T;
    const int nbytes = nv * T;
    int done = 0;
    if (words_ok) {                                            // mo is 4-aligned: pix0 * T is a multiple of 256 and the caller checked the rest
        const int nwords = nbytes >> 2;
        const uint32_t* sw = (const uint32_t*)s_msk;
        uint32_t* mw = (uint32_t*)mo;
        for (int i = tid; i < nwords; i += AUG_THREADS) mw[i] = sw[i];
        done = nwords << 2;
    }
    for (int i = done + tid; i < nbytes; i += AUG_THREADS) mo[i] = s_msk[i];
}

// pass 3: pixels.  A workgroup owns AUG_THREADS consecutive output pixels: each thread samples its pixel into LDS, then the workgroup writes its
// 3 * AUG_THREADS floats and T * AUG_THREADS mask bytes as contiguous runs (consecutive lanes, consecutive words).
template <int V>
__global__ __launch_bounds__(AUG_THREADS) void augment_render_kernel(const uint8_t* __restrict__ src_images, const uint8_t* __restrict__ src_masks,
                                                                     const double* __restrict__ params, const int* __restrict__ slotmap,
                                                                     double cval, float* __restrict__ images, uint8_t* __restrict__ masks,
                                                                     int H, int W, int T, int words_ok)
{
    __shared__ float s_img[AUG_THREADS * 3];
    __shared__ __attribute__((aligned(4))) uint8_t s_msk[AUG_THREADS * AUG_MAXT];
    __shared__ int s_slot[AUG_MAXT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long HW = (long long)H * W;
    const long long pix0 = (long long)blockIdx.x * AUG_THREADS, pix = pix0 + tid;
    const int nv = (int)((HW - pix0) < AUG_THREADS ? (HW - pix0) : AUG_THREADS);      // pixels of this workgroup inside the image
    if (tid < T) s_slot[tid] = slotmap[b * T + tid];
    __syncthreads();
    if (tid < nv) {
        const int py = (int)(pix / W), px = (int)(pix - (long long)py * W);
        const double* p = params + (long long)b * 8;
        double sx, sy;
        aug_source(p, px, py, sx, sy);
        // masks: nearest
        uint8_t* sm = s_msk + tid * T;
        for (int t = 0; t < T; ++t) sm[t] = 0;
        int ix, iy;
        if (aug_nearest(sx, sy, H, W, ix, iy)) {
            const uint8_t* mp = src_masks + ((long long)b * HW + (long long)iy * W + ix) * T;
            for (int w = 0; w < T; w += V) {
                const uint32_t word = aug_load<V>(mp + w);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int slot = s_slot[w + k];
                    if (slot >= 0 && ((word >> (8 * k)) & 0xffu) != 0) sm[slot] = 1;
                }
            }
        }
        aug_bilinear(src_images + (long long)b * HW * 3, sx, sy, p, cval, H, W, s_img + tid * 3);
    }
    __syncthreads();
    aug_write_runs(s_img, s_msk, images, masks, b, HW, pix0, nv, T, words_ok, tid);
}

// ---- mosaic ("Mosaic"): output pixel (x, y) of image b lies in tile q = (x >= cx) + 2 * (y >= cy) and is sampled from image
// quad_src[b][q] of the same batch through the row quad_rows[b][q] -- the three passes above with one more level of indirection.  The instance
// candidates of an image are the 4T pairs (q, t), q-major; the first T survivors take the output slots.
#define MOS_TILES 4

// tile, source image and source position of an output pixel.  A source index outside [0, B) (refused by DeviceAugmenter before the tables are
// uploaded) must not become an address: such a tile reads image 0 at a position whose every tap is outside the frame.
__device__ __forceinline__ int mosaic_source(const int32_t* __restrict__ quad_src, const double* __restrict__ quad_rows,
                                             const int32_t* __restrict__ centre, int b, int B, int x, int y, int& s, double& sx, double& sy)
{
    const int q = (x >= centre[2 * b] ? 1 : 0) + (y >= centre[2 * b + 1] ? 2 : 0);
    s = quad_src[b * MOS_TILES + q];
    aug_source(quad_rows + ((long long)b * MOS_TILES + q) * 8, x, y, sx, sy);
    if ((unsigned)s >= (unsigned)B) { s = 0; sx = sy = -4.0; }
    return q;
}

// pass 1 of the mosaic: augment_stats_kernel over the candidates (q, t).  A wave reduces only the tiles its pixels fall in (mostly one or two: 64
// neighbouring pixels of a row, four such runs a few rows apart), so the LDS table is zeroed first and a wave writes the entries it saw.
template <int V>
__global__ __launch_bounds__(AUG_THREADS) void mosaic_stats_kernel(const uint8_t* __restrict__ src_masks, const int32_t* __restrict__ src_ids,
                                                                   const int32_t* __restrict__ quad_src, const double* __restrict__ quad_rows,
                                                                   const int32_t* __restrict__ centre, int* __restrict__ stats,
                                                                   int B, int H, int W, int T)
{
    __shared__ int red[AUG_WAVES][MOS_TILES * AUG_MAXT][AUG_STAT_INTS];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long HW = (long long)H * W;
    for (int i = tid; i < AUG_WAVES * MOS_TILES * AUG_MAXT * AUG_STAT_INTS; i += AUG_THREADS) (&red[0][0][0])[i] = 0;
    int px[AUG_SPT], py[AUG_SPT], tile[AUG_SPT];               // tile -1: no output pixel (the ragged last workgroup)
    long long off[AUG_SPT];                                    // byte offset of the source pixel's slots, or -1: no source pixel
    unsigned seen = 0;                                         // tiles of this wave's pixels (wave-uniform: from ballots)
#pragma unroll
    for (int j = 0; j < AUG_SPT; ++j) {
        const long long pix = ((long long)blockIdx.x * AUG_SPT + j) * AUG_THREADS + tid;
        py[j] = (int)(pix / W); px[j] = (int)(pix - (long long)py[j] * W);
        off[j] = -1; tile[j] = -1;
        if (pix < HW) {
            double sx, sy;
            int s, ix, iy;
            tile[j] = mosaic_source(quad_src, quad_rows, centre, b, B, px[j], py[j], s, sx, sy);
            if (aug_nearest(sx, sy, H, W, ix, iy)) off[j] = (((long long)s * H + iy) * W + ix) * T;
        }
#pragma unroll
        for (int q = 0; q < MOS_TILES; ++q) seen |= __ballot(tile[j] == q) ? 1u << q : 0u;
    }
    __syncthreads();
    for (int w = 0; w < T; w += V) {
        uint32_t word[AUG_SPT];
#pragma unroll
        for (int j = 0; j < AUG_SPT; ++j) word[j] = off[j] >= 0 ? aug_load<V>(src_masks + off[j] + w) : 0u;
        for (int q = 0; q < MOS_TILES; ++q) {
            const int s = quad_src[b * MOS_TILES + q];
            if (!((seen >> q) & 1u) || (unsigned)s >= (unsigned)B) continue;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int t = w + k;
                const bool live = src_ids[s * T + t] != 0;
                int cnt = 0, a = 0, c = 0, d = 0, e = 0;
#pragma unroll
                for (int j = 0; j < AUG_SPT; ++j) {
                    const bool in = live && tile[j] == q && ((word[j] >> (8 * k)) & 0xffu) != 0;
                    cnt += __popcll(__ballot(in));
                    if (in) { a = max(a, W - px[j]); c = max(c, px[j] + 1); d = max(d, H - py[j]); e = max(e, py[j] + 1); }
                }
                if (cnt) {                                     // wave-uniform: it comes from ballots
                    a = aug_wave_max(a); c = aug_wave_max(c); d = aug_wave_max(d); e = aug_wave_max(e);
                    if (lane == 0) { int* r = red[wave][q * T + t]; r[0] = cnt; r[1] = a; r[2] = c; r[3] = d; r[4] = e; }
                }
            }
        }
    }
    __syncthreads();
    if (tid < MOS_TILES * T) {
        int cnt = 0, v[4] = {0, 0, 0, 0};
        for (int w = 0; w < AUG_WAVES; ++w) {
            cnt += red[w][tid][0];
            for (int k = 0; k < 4; ++k) v[k] = max(v[k], red[w][tid][1 + k]);
        }
        if (cnt) {
            int* st = stats + ((long long)b * MOS_TILES * T + tid) * AUG_STAT_INTS;
            atomicAdd(st, cnt);
            for (int k = 0; k < 4; ++k) atomicMax(st + 1 + k, v[k]);
        }
    }
}

// pass 2 of the mosaic (one workgroup per image): the candidates in q-major order; a live one with no pixel is dropped, the first T survivors take
// slots 0..T-1 in order, the others are discarded (slot -1: render leaves their pixels out) and counted.
__global__ void mosaic_encode_kernel(const int32_t* __restrict__ src_ids, const int32_t* __restrict__ quad_src, const int* __restrict__ stats,
                                     int* __restrict__ slotmap, int32_t* __restrict__ gt_ids, int32_t* __restrict__ gt_boxes,
                                     float* __restrict__ y_true, float* __restrict__ true_boxes, int32_t* __restrict__ dropped,
                                     const double* __restrict__ anchors, int B, int H, int W, int T, int G, int A, int C)
{
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const double cell_w = (double)W / G, cell_h = (double)H / G;
    int m = 0, tbi = 0, extra = 0;
    for (int k = 0; k < MOS_TILES * T; ++k) {
        const long long cand = (long long)b * MOS_TILES * T + k;
        const int* st = stats + cand * AUG_STAT_INTS;
        const int s = quad_src[b * MOS_TILES + k / T];
        const int cls = (unsigned)s < (unsigned)B ? src_ids[s * T + k % T] : 0;
        slotmap[cand] = -1;
        if (cls == 0 || st[0] <= 0) continue;
        if (m == T) { ++extra; continue; }
        slotmap[cand] = m;
        const int x1 = W - st[1], x2 = st[2], y1 = H - st[3], y2 = st[4];     // extract_bboxes: x2, y2 exclusive
        gt_ids[b * T + m] = cls;
        int32_t* gb = gt_boxes + ((long long)b * T + m) * 4;
        gb[0] = x1; gb[1] = y1; gb[2] = x2; gb[3] = y2;
        if (y_true) aug_encode_target(b, cls, x1, y1, x2, y2, cell_w, cell_h, anchors, y_true, true_boxes, tbi, T, G, A, C);
        ++m;
    }
    dropped[b] = extra;
}

// pass 3 of the mosaic: augment_render_kernel, each pixel from its tile's image through its tile's row
template <int V>
__global__ __launch_bounds__(AUG_THREADS) void mosaic_render_kernel(const uint8_t* __restrict__ src_images, const uint8_t* __restrict__ src_masks,
                                                                    const int32_t* __restrict__ quad_src, const double* __restrict__ quad_rows,
                                                                    const int32_t* __restrict__ centre, const int* __restrict__ slotmap,
                                                                    double cval, float* __restrict__ images, uint8_t* __restrict__ masks,
                                                                    int B, int H, int W, int T, int words_ok)
{
    __shared__ float s_img[AUG_THREADS * 3];
    __shared__ __attribute__((aligned(4))) uint8_t s_msk[AUG_THREADS * AUG_MAXT];
    __shared__ int s_slot[MOS_TILES * AUG_MAXT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long HW = (long long)H * W;
    const long long pix0 = (long long)blockIdx.x * AUG_THREADS, pix = pix0 + tid;
    const int nv = (int)((HW - pix0) < AUG_THREADS ? (HW - pix0) : AUG_THREADS);      // pixels of this workgroup inside the image
    if (tid < MOS_TILES * T) s_slot[tid] = slotmap[b * MOS_TILES * T + tid];
    __syncthreads();
    if (tid < nv) {
        const int py = (int)(pix / W), px = (int)(pix - (long long)py * W);
        double sx, sy;
        int s;
        const int q = mosaic_source(quad_src, quad_rows, centre, b, B, px, py, s, sx, sy);
        // masks: nearest
        uint8_t* sm = s_msk + tid * T;
        for (int t = 0; t < T; ++t) sm[t] = 0;
        int ix, iy;
        if (aug_nearest(sx, sy, H, W, ix, iy)) {
            const uint8_t* mp = src_masks + (((long long)s * H + iy) * W + ix) * T;
            for (int w = 0; w < T; w += V) {
                const uint32_t word = aug_load<V>(mp + w);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int slot = s_slot[q * T + w + k];
                    if (slot >= 0 && ((word >> (8 * k)) & 0xffu) != 0) sm[slot] = 1;
                }
            }
        }
        aug_bilinear(src_images + (long long)s * HW * 3, sx, sy, quad_rows + ((long long)b * MOS_TILES + q) * 8, cval, H, W, s_img + tid * 3);
    }
    __syncthreads();
    aug_write_runs(s_img, s_msk, images, masks, b, HW, pix0, nv, T, words_ok, tid);
}

// ---- copy-paste ("Copy-paste"): a second stage behind the passes above.  Image b receives the accepted instances of image d = donor[b]
// of the same, already augmented batch: their pixels replace the image's, their masks occlude its own.  The instance candidates of an image are the 2T
// pairs (own, t) then (donor, t); masks, boxes and targets are re-derived from the pasted masks by the same three passes.
#define CP_SIDES 2

// what a workgroup needs of the plan, derived by its first wave from the two id rows and select[b] (T <= 32: every set is one word)
struct CpPlan {
    int d;                   // the donor image, b itself when donor[b] lies outside [0, B) (nothing is accepted then: the index never becomes an address)
    uint32_t own;            // live own slots
    uint32_t acc;            // accepted donor slots: the lowest F = T - popcount(own) of the selected live ones
    int dropped;             // selected live donor slots beyond F
};

// Called by every thread of a workgroup of at least 64 threads; ends in a barrier.
__device__ __forceinline__ CpPlan cp_plan(const int32_t* __restrict__ ids, const int32_t* __restrict__ donor, const int32_t* __restrict__ select,
                                          int b, int B, int T, int* s_plan)
{
    if (threadIdx.x < 64) {
        const int t = threadIdx.x;
        const int d = donor[b];
        const bool valid = (unsigned)d < (unsigned)B;
        const uint32_t own = (uint32_t)__ballot(t < T && ids[(long long)b * T + t] != 0);
        const uint32_t dlive = (uint32_t)__ballot(t < T && valid && ids[(long long)(valid ? d : b) * T + t] != 0);
        if (t == 0) {
            const uint32_t sel = (uint32_t)select[b] & dlive;
            const int room = T - __popc(own);
            uint32_t acc = sel;
            while (__popc(acc) > room) acc &= ~(1u << (31 - __clz(acc)));     // the highest slots go first
            s_plan[0] = valid ? d : b; s_plan[1] = (int)own; s_plan[2] = (int)acc; s_plan[3] = __popc(sel) - __popc(acc);
        }
    }
    __syncthreads();
    CpPlan p;
    p.d = s_plan[0]; p.own = (uint32_t)s_plan[1]; p.acc = (uint32_t)s_plan[2]; p.dropped = s_plan[3];
    return p;
}

// the statistics of one candidate over a wave's AUG_SPT pixels each: ballot + popcount, shuffles, then the wave's LDS row (zeroed before)
#define CP_REDUCE(cand_, in_)                                                                                                                \
    do {                                                                                                                                     \
        int cnt = 0, a = 0, c = 0, d_ = 0, e = 0;                                                                                            \
        _Pragma("unroll") for (int j = 0; j < AUG_SPT; ++j) {                                                                                \
            const bool in = (in_);                                                                                                           \
            cnt += __popcll(__ballot(in));                                                                                                   \
            if (in) { a = max(a, W - px[j]); c = max(c, px[j] + 1); d_ = max(d_, H - py[j]); e = max(e, py[j] + 1); }                         \
        }                                                                                                                                    \
        if (cnt) {                                             /* wave-uniform: it comes from ballots */                                     \
            a = aug_wave_max(a); c = aug_wave_max(c); d_ = aug_wave_max(d_); e = aug_wave_max(e);                                             \
            if (lane == 0) { int* r = red[wave][cand_]; r[0] = cnt; r[1] = a; r[2] = c; r[3] = d_; r[4] = e; }                                \
        }                                                                                                                                    \
    } while (0)

// pass 1 of the copy-paste: augment_stats_kernel over the candidates (side, t) with no warp -- the donor's accepted slots first, which also gives the
// paste region U of the thread's pixels, then the own slots outside U.  A word none of whose slots is accepted (own: live) is not read: an image
// with nothing accepted reads no donor byte.
template <int V>
__global__ __launch_bounds__(AUG_THREADS) void copy_paste_stats_kernel(const uint8_t* __restrict__ masks, const int32_t* __restrict__ ids,
                                                                       const int32_t* __restrict__ donor, const int32_t* __restrict__ select,
                                                                       int* __restrict__ stats, int B, int H, int W, int T)
{
    __shared__ int red[AUG_WAVES][CP_SIDES * AUG_MAXT][AUG_STAT_INTS];
    __shared__ int s_plan[4];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long HW = (long long)H * W;
    for (int i = tid; i < AUG_WAVES * CP_SIDES * AUG_MAXT * AUG_STAT_INTS; i += AUG_THREADS) (&red[0][0][0])[i] = 0;
    const CpPlan plan = cp_plan(ids, donor, select, b, B, T, s_plan);          // (its barrier also covers the zeroed table)
    const uint8_t* mb = masks + (long long)b * HW * T;
    const uint8_t* md = masks + (long long)plan.d * HW * T;
    int px[AUG_SPT], py[AUG_SPT];
    long long off[AUG_SPT];                                    // byte offset of the pixel's slots, or -1: no pixel (the ragged last workgroup)
    bool pasted[AUG_SPT];                                      // U
#pragma unroll
    for (int j = 0; j < AUG_SPT; ++j) {
        const long long pix = ((long long)blockIdx.x * AUG_SPT + j) * AUG_THREADS + tid;
        py[j] = (int)(pix / W); px[j] = (int)(pix - (long long)py[j] * W);
        off[j] = pix < HW ? pix * T : -1;
        pasted[j] = false;
    }
    const uint32_t lanes_of_word = V == 4 ? 0xfu : V == 2 ? 0x3u : 0x1u;
    for (int w = 0; w < T; w += V) {
        if (!((plan.acc >> w) & lanes_of_word)) continue;      // workgroup-uniform
        uint32_t word[AUG_SPT];
#pragma unroll
        for (int j = 0; j < AUG_SPT; ++j) word[j] = off[j] >= 0 ? aug_load<V>(md + off[j] + w) : 0u;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int t = w + k;
            if (!((plan.acc >> t) & 1u)) continue;
#pragma unroll
            for (int j = 0; j < AUG_SPT; ++j) pasted[j] = pasted[j] || ((word[j] >> (8 * k)) & 0xffu) != 0;
            CP_REDUCE(T + t, ((word[j] >> (8 * k)) & 0xffu) != 0);
        }
    }
    for (int w = 0; w < T; w += V) {
        if (!((plan.own >> w) & lanes_of_word)) continue;
        uint32_t word[AUG_SPT];
#pragma unroll
        for (int j = 0; j < AUG_SPT; ++j) word[j] = off[j] >= 0 ? aug_load<V>(mb + off[j] + w) : 0u;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int t = w + k;
            if (!((plan.own >> t) & 1u)) continue;
            CP_REDUCE(t, !pasted[j] && ((word[j] >> (8 * k)) & 0xffu) != 0);
        }
    }
    __syncthreads();
    if (tid < CP_SIDES * T) {
        int cnt = 0, v[4] = {0, 0, 0, 0};
        for (int w = 0; w < AUG_WAVES; ++w) {
            cnt += red[w][tid][0];
            for (int k = 0; k < 4; ++k) v[k] = max(v[k], red[w][tid][1 + k]);
        }
        if (cnt) {
            int* st = stats + ((long long)b * CP_SIDES * T + tid) * AUG_STAT_INTS;
            atomicAdd(st, cnt);
            for (int k = 0; k < 4; ++k) atomicMax(st + 1 + k, v[k]);
        }
    }
}
#undef CP_REDUCE

// pass 2 of the copy-paste (one wave per image): the candidates own first; a live one with no pixel left is dropped and the survivors are compacted
// in order -- at most popcount(own) + popcount(acc) <= T of them.  The rejected donor slots were counted by the plan.
__global__ void copy_paste_encode_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ donor, const int32_t* __restrict__ select,
                                         const int* __restrict__ stats, int* __restrict__ slotmap, int32_t* __restrict__ gt_ids,
                                         int32_t* __restrict__ gt_boxes, float* __restrict__ y_true, float* __restrict__ true_boxes,
                                         int32_t* __restrict__ dropped, const double* __restrict__ anchors, int B, int H, int W, int T, int G, int A,
                                         int C)
{
    __shared__ int s_plan[4];
    const int b = blockIdx.x;
    const CpPlan plan = cp_plan(ids, donor, select, b, B, T, s_plan);
    if (threadIdx.x != 0) return;
    const double cell_w = (double)W / G, cell_h = (double)H / G;
    int m = 0, tbi = 0;
    for (int k = 0; k < CP_SIDES * T; ++k) {
        const long long cand = (long long)b * CP_SIDES * T + k;
        const int* st = stats + cand * AUG_STAT_INTS;
        const int t = k < T ? k : k - T;
        const bool live = ((k < T ? plan.own : plan.acc) >> t) & 1u;
        slotmap[cand] = -1;
        if (!live || st[0] <= 0 || m == T) continue;           // (m == T cannot happen: the plan accepted no more than the free slots)
        slotmap[cand] = m;
        const int cls = ids[(long long)(k < T ? b : plan.d) * T + t];
        const int x1 = W - st[1], x2 = st[2], y1 = H - st[3], y2 = st[4];     // extract_bboxes: x2, y2 exclusive
        gt_ids[b * T + m] = cls;
        int32_t* gb = gt_boxes + ((long long)b * T + m) * 4;
        gb[0] = x1; gb[1] = y1; gb[2] = x2; gb[3] = y2;
        if (y_true) aug_encode_target(b, cls, x1, y1, x2, y2, cell_w, cell_h, anchors, y_true, true_boxes, tbi, T, G, A, C);
        ++m;
    }
    dropped[b] = plan.dropped;
}

// pass 3 of the copy-paste: a workgroup owns AUG_THREADS consecutive pixels; each thread finds U of its pixel from the donor's accepted slots, takes
// the pixel's three floats from the donor under U and from the image itself elsewhere (a copy, bit for bit), and writes its mask bytes through the
// slot map into LDS; then the contiguous runs leave as in the first stage.
template <int V>
__global__ __launch_bounds__(AUG_THREADS) void copy_paste_render_kernel(const float* __restrict__ src_images, const uint8_t* __restrict__ src_masks,
                                                                        const int32_t* __restrict__ ids, const int32_t* __restrict__ donor,
                                                                        const int32_t* __restrict__ select, const int* __restrict__ slotmap,
                                                                        float* __restrict__ images, uint8_t* __restrict__ masks,
                                                                        int B, int H, int W, int T, int words_ok)
{
    __shared__ float s_img[AUG_THREADS * 3];
    __shared__ __attribute__((aligned(4))) uint8_t s_msk[AUG_THREADS * AUG_MAXT];
    __shared__ int s_slot[CP_SIDES * AUG_MAXT];
    __shared__ int s_plan[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long HW = (long long)H * W;
    const long long pix0 = (long long)blockIdx.x * AUG_THREADS, pix = pix0 + tid;
    const int nv = (int)((HW - pix0) < AUG_THREADS ? (HW - pix0) : AUG_THREADS);      // pixels of this workgroup inside the image
    if (tid < CP_SIDES * T) s_slot[tid] = slotmap[b * CP_SIDES * T + tid];
    const CpPlan plan = cp_plan(ids, donor, select, b, B, T, s_plan);
    const uint32_t lanes_of_word = V == 4 ? 0xfu : V == 2 ? 0x3u : 0x1u;
    if (tid < nv) {
        uint8_t* sm = s_msk + tid * T;
        for (int t = 0; t < T; ++t) sm[t] = 0;
        bool pasted = false;
        const uint8_t* mp = src_masks + ((long long)plan.d * HW + pix) * T;
        for (int w = 0; w < T; w += V) {
            if (!((plan.acc >> w) & lanes_of_word)) continue;
            const uint32_t word = aug_load<V>(mp + w);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (!((plan.acc >> (w + k)) & 1u) || ((word >> (8 * k)) & 0xffu) == 0) continue;
                pasted = true;
                const int slot = s_slot[T + w + k];
                if (slot >= 0) sm[slot] = 1;
            }
        }
        if (!pasted) {
            mp = src_masks + ((long long)b * HW + pix) * T;
            for (int w = 0; w < T; w += V) {
                if (!((plan.own >> w) & lanes_of_word)) continue;
                const uint32_t word = aug_load<V>(mp + w);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int slot = s_slot[w + k];
                    if (((plan.own >> (w + k)) & 1u) && slot >= 0 && ((word >> (8 * k)) & 0xffu) != 0) sm[slot] = 1;
                }
            }
        }
        const float* ip = src_images + ((long long)(pasted ? plan.d : b) * HW + pix) * 3;
        s_img[tid * 3] = ip[0]; s_img[tid * 3 + 1] = ip[1]; s_img[tid * 3 + 2] = ip[2];
    }
    __syncthreads();
    aug_write_runs(s_img, s_msk, images, masks, b, HW, pix0, nv, T, words_ok, tid);
}

// [p, p + n) and [q, q + m) share a byte
static bool cp_overlap(const void* p, size_t n, const void* q, size_t m)
{
    const uintptr_t a = (uintptr_t)p, c = (uintptr_t)q;
    return p && q && a < c + m && c < a + n;
}

extern "C" {

size_t myolo_augment_batch_ws_bytes(int B, int T)
{
    if (B <= 0 || T <= 0) return 0;
    return (size_t)B * T * (AUG_STAT_INTS + 1) * sizeof(int);
}

int myolo_augment_batch(const uint8_t* src_images, const uint8_t* src_masks, const int32_t* src_class_ids, const double* params, double cval,
                        const double* anchors, float* images, uint8_t* gt_masks, int32_t* gt_boxes, int32_t* gt_class_ids, float* y_true,
                        float* true_boxes, int B, int H, int W, int T, int G, int A, int C, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(src_images && src_masks && src_class_ids && params && images && gt_masks && gt_boxes && gt_class_ids,
                  "augment_batch: null pointer");
    MYOLO_REQUIRE((y_true != nullptr) == (true_boxes != nullptr), "augment_batch: y_true and true_boxes are given together or not at all");
    MYOLO_REQUIRE(!y_true || anchors, "augment_batch: targets need the anchors");
    MYOLO_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) - AUG_THREADS * AUG_SPT, "augment_batch: bad sizes (B=%d, H=%d, W=%d)", B, H, W);
    MYOLO_REQUIRE(T > 0 && T <= AUG_MAXT, "augment_batch: need 1 <= T <= %d (got %d)", AUG_MAXT, T);
    MYOLO_REQUIRE(!y_true || (G > 0 && A > 0 && C > 0), "augment_batch: bad target sizes (G=%d, A=%d, C=%d)", G, A, C);
    MYOLO_NEED_WS(myolo_augment_batch_ws_bytes(B, T));
    int* stats = (int*)ws;
    int* slotmap = stats + (size_t)B * T * AUG_STAT_INTS;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(stats, 0, (size_t)B * T * AUG_STAT_INTS * sizeof(int), s);
    (void)hipMemsetAsync(gt_boxes, 0, (size_t)B * T * 4 * sizeof(int32_t), s);
    (void)hipMemsetAsync(gt_class_ids, 0, (size_t)B * T * sizeof(int32_t), s);
    if (y_true) {
        (void)hipMemsetAsync(y_true, 0, (size_t)B * G * G * A * (5 + C) * sizeof(float), s);
        (void)hipMemsetAsync(true_boxes, 0, (size_t)B * T * 4 * sizeof(float), s);
    }
    const long long HW = (long long)H * W;
    const dim3 grid((unsigned)((HW + AUG_THREADS - 1) / AUG_THREADS), B), grid1((unsigned)((HW + AUG_THREADS * AUG_SPT - 1) / (AUG_THREADS * AUG_SPT)), B);
    // bytes per load of a pixel's T mask slots: every pixel's run starts on a multiple of T from the base pointer
    const int V = (T % 4 == 0 && ((uintptr_t)src_masks & 3) == 0) ? 4 : (T % 2 == 0 && ((uintptr_t)src_masks & 1) == 0) ? 2 : 1;
    // word stores of the mask bytes need every workgroup's run to start on a word: the base pointer and each image's H*W*T bytes
    const int words_ok = (((uintptr_t)gt_masks & 3) == 0 && ((HW * T) & 3) == 0) ? 1 : 0;
#define AUG_LAUNCH(V_)                                                                                                                       \
    do {                                                                                                                                     \
        hipLaunchKernelGGL(augment_stats_kernel<V_>, grid1, dim3(AUG_THREADS), 0, s, src_masks, src_class_ids, params, stats, H, W, T);      \
        hipLaunchKernelGGL(augment_encode_kernel, dim3(B), dim3(64), 0, s, src_class_ids, (const int*)stats, slotmap, gt_class_ids, gt_boxes, \
                           y_true, true_boxes, anchors, H, W, T, G, A, C);                                                                  \
        hipLaunchKernelGGL(augment_render_kernel<V_>, grid, dim3(AUG_THREADS), 0, s, src_images, src_masks, params, (const int*)slotmap, cval, \
                           images, gt_masks, H, W, T, words_ok);                                                                             \
    } while (0)
    if (V == 4) AUG_LAUNCH(4);
    else if (V == 2) AUG_LAUNCH(2);
    else AUG_LAUNCH(1);
#undef AUG_LAUNCH
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

size_t myolo_mosaic_batch_ws_bytes(int B, int T)
{
    if (B <= 0 || T <= 0) return 0;
    return (size_t)B * MOS_TILES * T * (AUG_STAT_INTS + 1) * sizeof(int);
}

int myolo_mosaic_batch(const uint8_t* src_images, const uint8_t* src_masks, const int32_t* src_class_ids, const int32_t* quad_src,
                       const double* quad_rows, const int32_t* centre, double cval, const double* anchors, float* images, uint8_t* gt_masks,
                       int32_t* gt_boxes, int32_t* gt_class_ids, float* y_true, float* true_boxes, int32_t* dropped, int B, int H, int W, int T,
                       int G, int A, int C, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(src_images && src_masks && src_class_ids && quad_src && quad_rows && centre && images && gt_masks && gt_boxes && gt_class_ids &&
                  dropped, "mosaic_batch: null pointer");
    MYOLO_REQUIRE((y_true != nullptr) == (true_boxes != nullptr), "mosaic_batch: y_true and true_boxes are given together or not at all");
    MYOLO_REQUIRE(!y_true || anchors, "mosaic_batch: targets need the anchors");
    MYOLO_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) - AUG_THREADS * AUG_SPT, "mosaic_batch: bad sizes (B=%d, H=%d, W=%d)", B, H, W);
    MYOLO_REQUIRE(T > 0 && T <= AUG_MAXT, "mosaic_batch: need 1 <= T <= %d (got %d)", AUG_MAXT, T);
    MYOLO_REQUIRE(!y_true || (G > 0 && A > 0 && C > 0), "mosaic_batch: bad target sizes (G=%d, A=%d, C=%d)", G, A, C);
    MYOLO_REQUIRE(ws && ws_bytes >= myolo_mosaic_batch_ws_bytes(B, T), "mosaic_batch: workspace too small (%zu bytes, need %zu)", ws_bytes,
                  myolo_mosaic_batch_ws_bytes(B, T));
    const size_t cands = (size_t)B * MOS_TILES * T;
    int* stats = (int*)ws;
    int* slotmap = stats + cands * AUG_STAT_INTS;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(stats, 0, cands * AUG_STAT_INTS * sizeof(int), s);
    (void)hipMemsetAsync(gt_boxes, 0, (size_t)B * T * 4 * sizeof(int32_t), s);
    (void)hipMemsetAsync(gt_class_ids, 0, (size_t)B * T * sizeof(int32_t), s);
    if (y_true) {
        (void)hipMemsetAsync(y_true, 0, (size_t)B * G * G * A * (5 + C) * sizeof(float), s);
        (void)hipMemsetAsync(true_boxes, 0, (size_t)B * T * 4 * sizeof(float), s);
    }
    const long long HW = (long long)H * W;
    const dim3 grid((unsigned)((HW + AUG_THREADS - 1) / AUG_THREADS), B), grid1((unsigned)((HW + AUG_THREADS * AUG_SPT - 1) / (AUG_THREADS * AUG_SPT)), B);
    const int V = (T % 4 == 0 && ((uintptr_t)src_masks & 3) == 0) ? 4 : (T % 2 == 0 && ((uintptr_t)src_masks & 1) == 0) ? 2 : 1;
    const int words_ok = (((uintptr_t)gt_masks & 3) == 0 && ((HW * T) & 3) == 0) ? 1 : 0;
#define MOS_LAUNCH(V_)                                                                                                                       \
    do {                                                                                                                                     \
        hipLaunchKernelGGL(mosaic_stats_kernel<V_>, grid1, dim3(AUG_THREADS), 0, s, src_masks, src_class_ids, quad_src, quad_rows, centre, stats, \
                           B, H, W, T);                                                                                                      \
        hipLaunchKernelGGL(mosaic_encode_kernel, dim3(B), dim3(64), 0, s, src_class_ids, quad_src, (const int*)stats, slotmap, gt_class_ids,  \
                           gt_boxes, y_true, true_boxes, dropped, anchors, B, H, W, T, G, A, C);                                             \
        hipLaunchKernelGGL(mosaic_render_kernel<V_>, grid, dim3(AUG_THREADS), 0, s, src_images, src_masks, quad_src, quad_rows, centre,      \
                           (const int*)slotmap, cval, images, gt_masks, B, H, W, T, words_ok);                                               \
    } while (0)
    if (V == 4) MOS_LAUNCH(4);
    else if (V == 2) MOS_LAUNCH(2);
    else MOS_LAUNCH(1);
#undef MOS_LAUNCH
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

size_t myolo_copy_paste_batch_ws_bytes(int B, int T)
{
    if (B <= 0 || T <= 0) return 0;
    return (size_t)B * CP_SIDES * T * (AUG_STAT_INTS + 1) * sizeof(int);
}

int myolo_copy_paste_batch(const float* src_images, const uint8_t* src_masks, const int32_t* src_class_ids, const int32_t* donor,
                           const int32_t* select, const double* anchors, float* images, uint8_t* gt_masks, int32_t* gt_boxes,
                           int32_t* gt_class_ids, float* y_true, float* true_boxes, int32_t* dropped, int B, int H, int W, int T, int G, int A, int C,
                           void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(src_images && src_masks && src_class_ids && donor && select && images && gt_masks && gt_boxes && gt_class_ids && dropped,
                  "copy_paste_batch: null pointer");
    MYOLO_REQUIRE((y_true != nullptr) == (true_boxes != nullptr), "copy_paste_batch: y_true and true_boxes are given together or not at all");
    MYOLO_REQUIRE(!y_true || anchors, "copy_paste_batch: targets need the anchors");
    MYOLO_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) - AUG_THREADS * AUG_SPT, "copy_paste_batch: bad sizes (B=%d, H=%d, W=%d)", B, H, W);
    MYOLO_REQUIRE(T > 0 && T <= AUG_MAXT, "copy_paste_batch: need 1 <= T <= %d (got %d)", AUG_MAXT, T);
    MYOLO_REQUIRE(!y_true || (G > 0 && A > 0 && C > 0), "copy_paste_batch: bad target sizes (G=%d, A=%d, C=%d)", G, A, C);
    const long long HW = (long long)H * W;
    {   // a donor is read in its state before the paste, while other images of the batch are being written: no output may lie over an input
        const void* in[5] = {src_images, src_masks, src_class_ids, donor, select};
        const size_t in_bytes[5] = {(size_t)B * HW * 3 * sizeof(float), (size_t)B * HW * T, (size_t)B * T * sizeof(int32_t), (size_t)B * sizeof(int32_t),
                                    (size_t)B * sizeof(int32_t)};
        const void* out[7] = {images, gt_masks, gt_boxes, gt_class_ids, y_true, true_boxes, dropped};
        const size_t out_bytes[7] = {in_bytes[0], in_bytes[1], (size_t)B * T * 4 * sizeof(int32_t), in_bytes[2],
                                     y_true ? (size_t)B * G * G * A * (5 + C) * sizeof(float) : 0, (size_t)B * T * 4 * sizeof(float), in_bytes[3]};
        for (int i = 0; i < 5; ++i)
            for (int o = 0; o < 7; ++o)
                MYOLO_REQUIRE(!cp_overlap(in[i], in_bytes[i], out[o], out_bytes[o]), "copy_paste_batch: output %d lies over input %d", o, i);
    }
    MYOLO_REQUIRE(ws && ws_bytes >= myolo_copy_paste_batch_ws_bytes(B, T), "copy_paste_batch: workspace too small (%zu bytes, need %zu)", ws_bytes,
                  myolo_copy_paste_batch_ws_bytes(B, T));
    const size_t cands = (size_t)B * CP_SIDES * T;
    int* stats = (int*)ws;
    int* slotmap = stats + cands * AUG_STAT_INTS;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(stats, 0, cands * AUG_STAT_INTS * sizeof(int), s);
    (void)hipMemsetAsync(gt_boxes, 0, (size_t)B * T * 4 * sizeof(int32_t), s);
    (void)hipMemsetAsync(gt_class_ids, 0, (size_t)B * T * sizeof(int32_t), s);
    if (y_true) {
        (void)hipMemsetAsync(y_true, 0, (size_t)B * G * G * A * (5 + C) * sizeof(float), s);
        (void)hipMemsetAsync(true_boxes, 0, (size_t)B * T * 4 * sizeof(float), s);
    }
    const dim3 grid((unsigned)((HW + AUG_THREADS - 1) / AUG_THREADS), B), grid1((unsigned)((HW + AUG_THREADS * AUG_SPT - 1) / (AUG_THREADS * AUG_SPT)), B);
    const int V = (T % 4 == 0 && ((uintptr_t)src_masks & 3) == 0) ? 4 : (T % 2 == 0 && ((uintptr_t)src_masks & 1) == 0) ? 2 : 1;
    const int words_ok = (((uintptr_t)gt_masks & 3) == 0 && ((HW * T) & 3) == 0) ? 1 : 0;
#define CP_LAUNCH(V_)                                                                                                                        \
    do {                                                                                                                                     \
        hipLaunchKernelGGL(copy_paste_stats_kernel<V_>, grid1, dim3(AUG_THREADS), 0, s, src_masks, src_class_ids, donor, select, stats, B, H, W, T); \
        hipLaunchKernelGGL(copy_paste_encode_kernel, dim3(B), dim3(64), 0, s, src_class_ids, donor, select, (const int*)stats, slotmap,       \
                           gt_class_ids, gt_boxes, y_true, true_boxes, dropped, anchors, B, H, W, T, G, A, C);                               \
        hipLaunchKernelGGL(copy_paste_render_kernel<V_>, grid, dim3(AUG_THREADS), 0, s, src_images, src_masks, src_class_ids, donor, select,  \
                           (const int*)slotmap, images, gt_masks, B, H, W, T, words_ok);                                                     \
    } while (0)
    if (V == 4) CP_LAUNCH(4);
    else if (V == 2) CP_LAUNCH(2);
    else CP_LAUNCH(1);
#undef CP_LAUNCH
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

}  // extern "C"
