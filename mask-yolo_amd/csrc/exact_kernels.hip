// Kernels whose outputs feed INTEGER decisions (positive/negative ROI partition, argmax class,
// no-object mask) and therefore must agree bit-for-bit with the CPU restatement:
//   yolo_decode / yolo_detections  (DecodeYOLOLayer model.py:1442-1473, DetectionsLayer :1493-1538)
//   mask_targets                   (detect_mask_target_graph model.py:457-602 + helpers)
//   yolo_loss fwd+bwd              (yolo_custom_loss model.py:86-242)
// This translation unit is compiled with -ffp-contract=off: every float expression below is a
// sequence of individually rounded IEEE-754 binary32 operations in source order, and exp/sigmoid
// are the explicit polynomial of exact_math.h (same operation sequence as the oracle's det_expf).
#include "myolo_common.h"
#include "exact_math.h"

// ---------------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void decode_box(const float* __restrict__ p, const float* __restrict__ anchors, int a, int col,
                                           int row, float Gf, float* out4)
{
    const float x = (myolo_sigmoidf(p[0]) + (float)col) / Gf;
    const float y = (myolo_sigmoidf(p[1]) + (float)row) / Gf;
    const float w = (myolo_expf(p[2]) * anchors[2 * a + 0]) / Gf;
    const float h = (myolo_expf(p[3]) * anchors[2 * a + 1]) / Gf;
    const float hw = w / 2.0f, hh = h / 2.0f;
    out4[0] = x - hw;
    out4[1] = y - hh;
    out4[2] = x + hw;
    out4[3] = y + hh;
}

__global__ void yolo_decode_kernel(const float* __restrict__ yp, const float* __restrict__ anchors, float* __restrict__ out,
                                   int total, int G, int A, int D, int det)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int a = i % A;
    const int col = (i / A) % G;
    const int row = (i / (A * G)) % G;
    const float* p = yp + (long long)i * D;
    float b[4];
    decode_box(p, anchors, a, col, row, (float)G, b);
    if (!det) {
        float* o = out + (long long)i * 4;
        o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
    } else {
        float* o = out + (long long)i * 6;
        o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
        o[4] = myolo_sigmoidf(p[4]);
        int best = 0;
        float bv = p[5];
        for (int k = 1; k < D - 5; ++k)
            if (p[5 + k] > bv) { bv = p[5 + k]; best = k; }     // first maximum wins (tf.argmax)
        o[5] = (float)best;
    }
}

// ---------------------------------------------------------------------------------------
// mask targets: one block per image
// ---------------------------------------------------------------------------------------
#define MT_MAXT 64
#define MT_MAXR 2048
__global__ __launch_bounds__(256) void mask_targets_kernel(const float* __restrict__ proposals, const int32_t* __restrict__ gt_ids,
                                                           const int32_t* __restrict__ gt_boxes, const uint8_t* __restrict__ gt_masks,
                                                           float* __restrict__ rois, int32_t* __restrict__ tcls,
                                                           float* __restrict__ tmasks, int32_t* __restrict__ npos_out,
                                                           int R, int T, int H, int W, int mh, int mw)
{
    __shared__ float gtb[MT_MAXT][4];
    __shared__ int keep[MT_MAXT];
    __shared__ int nkeep_s;
    __shared__ unsigned char posf[MT_MAXR];
    __shared__ short arg[MT_MAXR];
    __shared__ short dest[MT_MAXR];
    __shared__ short src_of_dest[MT_MAXR];
    __shared__ int npos_s;
    __shared__ int wcnt[2][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* prop = proposals + (long long)b * R * 4;

    // norm_boxes_graph (model.py:1405-1408): (box - [0,0,1,1]) / ([H,W,H,W] - 1)   (reference splits (H,W) as w,h)
    if (tid < T) {
        const int32_t* bp = gt_boxes + ((long long)b * T + tid) * 4;
        gtb[tid][0] = ((float)bp[0] - 0.0f) / (float)(H - 1);
        gtb[tid][1] = ((float)bp[1] - 0.0f) / (float)(W - 1);
        gtb[tid][2] = ((float)bp[2] - 1.0f) / (float)(H - 1);
        gtb[tid][3] = ((float)bp[3] - 1.0f) / (float)(W - 1);
    }
    __syncthreads();
    if (tid == 0) {   // trim_zeros_graph (model.py:1418): keep rows whose |.| sum is non-zero
        int n = 0;
        for (int g = 0; g < T; ++g) {
            const float s = fabsf(gtb[g][0]) + fabsf(gtb[g][1]) + fabsf(gtb[g][2]) + fabsf(gtb[g][3]);
            if (s != 0.0f) keep[n++] = g;
        }
        nkeep_s = n;
    }
    __syncthreads();
    const int nkeep = nkeep_s;
    // overlaps_graph (model.py:438-451) + reduce_max / argmax over the kept GT boxes
    for (int r = tid; r < R; r += blockDim.x) {
        const float bx1 = prop[r * 4 + 0], by1 = prop[r * 4 + 1], bx2 = prop[r * 4 + 2], by2 = prop[r * 4 + 3];
        const float a1 = (by2 - by1) * (bx2 - bx1);
        float best = -INFINITY;
        int bi = 0;
        bool any_nan = false;
        for (int k = 0; k < nkeep; ++k) {
            const int g = keep[k];
            const float x1 = fmaxf(bx1, gtb[g][0]), y1 = fmaxf(by1, gtb[g][1]);
            const float x2 = fminf(bx2, gtb[g][2]), y2 = fminf(by2, gtb[g][3]);
            const float inter = fmaxf(x2 - x1, 0.0f) * fmaxf(y2 - y1, 0.0f);
            const float a2 = (gtb[g][3] - gtb[g][1]) * (gtb[g][2] - gtb[g][0]);
            const float uni = a1 + a2 - inter;
            const float iou = inter / uni;
            if (iou != iou) any_nan = true;                   // 0 / 0: a zero-area proposal against a zero-area kept box
            else if (iou > best) { best = iou; bi = k; }      // first maximum among the non-NaN entries (read for positives only)
        }
        // reduce_max propagates a NaN (the oracle's ov.max(1)): one NaN IoU in the row makes the row's maximum NaN
        if (any_nan) best = NAN;
        // positive: max IoU >= 0.5 ; negative: < 0.5 ; NaN belongs to neither (2 = dropped, the tail of the outputs is zero-padded)
        posf[r] = (best >= 0.5f) ? 1 : ((best < 0.5f) ? 0 : 2);
        arg[r] = (short)bi;
    }
    __syncthreads();
    // stable partition: positives first, then negatives, index order kept -- ranks by ballots over chunks of 256 proposals (a single thread walking
    // the R proposals four times through LDS took ~15 us of the step's critical path)
    {
        const int lane = tid & 63, wave = tid >> 6;
        const unsigned long long lower = (1ull << lane) - 1ull;
        int base_p = 0, base_n = 0;
        for (int r0 = 0; r0 < R; r0 += 256) {
            const int r = r0 + tid;
            const int f = r < R ? posf[r] : 2;
            const unsigned long long bp = __ballot(f == 1), bn = __ballot(f == 0);
            if (lane == 0) { wcnt[0][wave] = __popcll(bp); wcnt[1][wave] = __popcll(bn); }
            __syncthreads();
            int offp = base_p, offn = base_n;
            for (int w2 = 0; w2 < wave; ++w2) { offp += wcnt[0][w2]; offn += wcnt[1][w2]; }
            if (f == 1) dest[r] = (short)(offp + __popcll(bp & lower));
            else if (f == 0) dest[r] = (short)(-2 - (offn + __popcll(bn & lower)));         // negatives: rank among negatives, shifted below
            else if (r < R) dest[r] = -1;
            base_p += wcnt[0][0] + wcnt[0][1] + wcnt[0][2] + wcnt[0][3];
            base_n += wcnt[1][0] + wcnt[1][1] + wcnt[1][2] + wcnt[1][3];
            __syncthreads();
        }
        if (tid == 0) { npos_s = base_p; if (blockIdx.y == 0) npos_out[b] = base_p; }
        for (int d = tid; d < R; d += blockDim.x) src_of_dest[d] = -1;
        __syncthreads();
        for (int r = tid; r < R; r += blockDim.x) {
            int d = dest[r];
            if (d <= -2) { d = base_p + (-2 - d); dest[r] = (short)d; }
            if (d >= 0) src_of_dest[d] = (short)r;
        }
    }
    __syncthreads();
    const int npos = npos_s;
    // rois + class ids
    // (every workgroup of an image repeats the matching above -- a few microseconds -- and fills its share of the image's target masks, 115 000
    // values at 28 x 28 and R = 147; the first one also writes the ROIs and class ids)
    if (blockIdx.y == 0)
    for (int d = tid; d < R; d += blockDim.x) {
        const int r = src_of_dest[d];
        float* o = rois + ((long long)b * R + d) * 4;
        if (r >= 0) {
            o[0] = prop[r * 4 + 0]; o[1] = prop[r * 4 + 1]; o[2] = prop[r * 4 + 2]; o[3] = prop[r * 4 + 3];
        } else {
            o[0] = o[1] = o[2] = o[3] = 0.0f;
        }
        int cls = 0;
        if (r >= 0 && d < npos) cls = gt_ids[(long long)b * T + keep[arg[r]]];
        tcls[(long long)b * R + d] = cls;
    }
    // mask targets: crop_and_resize(gt_mask[g], [y1,x1,y2,x2], mh x mw) then tf.round (model.py:558-589)
    const int msz = mh * mw;
    float* tm = tmasks + (long long)b * R * msz;
    const int per = (R * msz + (int)gridDim.y - 1) / (int)gridDim.y;
    const int i_lo = (int)blockIdx.y * per, i_hi = i_lo + per < R * msz ? i_lo + per : R * msz;
    for (int i = i_lo + tid; i < i_hi; i += blockDim.x) {
        const int d = i / msz;
        float v = 0.0f;
        if (d < npos) {
            const int r = src_of_dest[d];
            const int g = keep[arg[r]];
            const int py = (i - d * msz) / mw, px = (i - d * msz) % mw;
            const float bx1 = prop[r * 4 + 0], by1 = prop[r * 4 + 1], bx2 = prop[r * 4 + 2], by2 = prop[r * 4 + 3];
            float iny, inx;
            const float sy = (by2 - by1) * (float)(H - 1) / (float)(mh - 1);
            iny = by1 * (float)(H - 1) + (float)py * sy;
            const float sx = (bx2 - bx1) * (float)(W - 1) / (float)(mw - 1);
            inx = bx1 * (float)(W - 1) + (float)px * sx;
            const bool ok = !(iny < 0.0f || iny > (float)(H - 1)) && !(inx < 0.0f || inx > (float)(W - 1));
            if (ok) {
                const int ty = (int)floorf(iny), byy = (int)ceilf(iny);
                const int lx = (int)floorf(inx), rx = (int)ceilf(inx);
                const float wy = iny - (float)ty, wx = inx - (float)lx;
                const uint8_t* mp = gt_masks + (long long)b * H * W * T + g;
                const float tl = (float)(mp[((long long)ty * W + lx) * T] != 0), tr = (float)(mp[((long long)ty * W + rx) * T] != 0);
                const float bl = (float)(mp[((long long)byy * W + lx) * T] != 0), br = (float)(mp[((long long)byy * W + rx) * T] != 0);
                const float top = tl + (tr - tl) * wx;
                const float bot = bl + (br - bl) * wx;
                v = rintf(top + (bot - top) * wy);          // round half to even
            }
        }
        tm[i] = v;
    }
}

// ---------------------------------------------------------------------------------------
// YOLO loss, forward + gradient.  Single block (B*G*G*A is a few thousand boxes).
// ---------------------------------------------------------------------------------------
struct IouOut { float iou, inter, uni, dw, dh; float pminx, pminy, pmaxx, pmaxy, tminx, tminy, tmaxx, tmaxy; };

__device__ __forceinline__ float iou_centre(float px, float py, float pw, float ph, float tx, float ty, float tw, float th, IouOut* o)
{
    const float pminx = px - pw / 2.0f, pmaxx = px + pw / 2.0f, pminy = py - ph / 2.0f, pmaxy = py + ph / 2.0f;
    const float tminx = tx - tw / 2.0f, tmaxx = tx + tw / 2.0f, tminy = ty - th / 2.0f, tmaxy = ty + th / 2.0f;
    const float dw = fminf(pmaxx, tmaxx) - fmaxf(pminx, tminx);
    const float dh = fminf(pmaxy, tmaxy) - fmaxf(pminy, tminy);
    const float iw = fmaxf(dw, 0.0f), ih = fmaxf(dh, 0.0f);
    const float inter = iw * ih;
    const float uni = pw * ph + tw * th - inter;
    const float iou = inter / uni;
    if (o) {
        o->iou = iou; o->inter = inter; o->uni = uni; o->dw = dw; o->dh = dh;
        o->pminx = pminx; o->pminy = pminy; o->pmaxx = pmaxx; o->pmaxy = pmaxy;
        o->tminx = tminx; o->tminy = tminy; o->tmaxx = tmaxx; o->tmaxy = tmaxy;
    }
    return iou;
}

struct LossArgs {
    const float* yt; const float* yp; const float* tb; const float* anchors; const float* cw;
    float obj, noobj, coord, cls, lw;
    float* out; float* grad;
    int B, G, A, C, T;
    int warm;                  // the warm-up branch of model.py:193-207
};

#define LOSS_NACC 9   // sum_xy, sum_wh, sum_conf, sum_cls, n_coord, n_conf, n_cls, nb_true, nb_pred
__global__ __launch_bounds__(256) void yolo_loss_kernel(LossArgs a)
{
    __shared__ double red[LOSS_NACC][256];
    __shared__ double tot[LOSS_NACC];
    const int D = 5 + a.C;
    const int total = a.B * a.G * a.G * a.A;
    const int tid = threadIdx.x;
    double acc[LOSS_NACC];
    for (int k = 0; k < LOSS_NACC; ++k) acc[k] = 0;

    for (int pass = 0; pass < 2; ++pass) {
        for (int i = tid; i < total; i += blockDim.x) {
            const int an = i % a.A;
            const int col = (i / a.A) % a.G;
            const int row = (i / (a.A * a.G)) % a.G;
            const int b = i / (a.A * a.G * a.G);
            const float* p = a.yp + (long long)i * D;
            const float* t = a.yt + (long long)i * D;
            const float sx = myolo_sigmoidf(p[0]), sy = myolo_sigmoidf(p[1]);
            const float px = sx + (float)col, py = sy + (float)row;
            const float pw = myolo_expf(p[2]) * a.anchors[2 * an], ph = myolo_expf(p[3]) * a.anchors[2 * an + 1];
            const float pc = myolo_sigmoidf(p[4]);
            const float t4 = t[4];
            IouOut io;
            const float iou1 = iou_centre(px, py, pw, ph, t[0], t[1], t[2], t[3], &io);
            const float tconf = iou1 * t4;
            int tcls = 0;
            float tv = t[5];
            for (int k = 1; k < a.C; ++k)
                if (t[5 + k] > tv) { tv = t[5 + k]; tcls = k; }
            float best = -INFINITY;
            for (int k = 0; k < a.T; ++k) {
                const float* q = a.tb + ((long long)b * a.T + k) * 4;
                const float v = iou_centre(px, py, pw, ph, q[0], q[1], q[2], q[3], nullptr);
                if (v > best) best = v;
            }
            float coord_mask = t4 * a.coord;
            // warm-up (model.py:193-207, while seen < WARM_UP_BATCHES): a predictor without a box is pulled to its cell centre and its anchor's size,
            // and every predictor's coordinate terms count with weight 1; the IoU / confidence / class terms above keep the plain targets
            float txl = t[0], tyl = t[1], twl = t[2], thl = t[3];
            if (a.warm) {
                const float nob = (coord_mask < a.coord / 2.0f) ? 1.0f : 0.0f;
                txl = t[0] + (0.5f + (float)col) * nob;
                tyl = t[1] + (0.5f + (float)row) * nob;
                twl = t[2] + 1.0f * a.anchors[2 * an] * nob;
                thl = t[3] + 1.0f * a.anchors[2 * an + 1] * nob;
                coord_mask = 1.0f;
            }
            const float conf_mask = ((best < 0.6f) ? 1.0f : 0.0f) * (1.0f - t4) * a.noobj + t4 * a.obj;
            const float class_mask = t4 * a.cw[tcls] * a.cls;
            // softmax CE over class logits
            float mx = p[5];
            for (int k = 1; k < a.C; ++k) mx = fmaxf(mx, p[5 + k]);
            float se = 0.0f;
            for (int k = 0; k < a.C; ++k) se += expf(p[5 + k] - mx);
            const float lse = logf(se) + mx;
            if (pass == 0) {
                const float ex = txl - px, ey = tyl - py, ew = twl - pw, eh = thl - ph, ec = tconf - pc;
                acc[0] += (double)((ex * ex + ey * ey) * coord_mask);
                acc[1] += (double)((ew * ew + eh * eh) * coord_mask);
                acc[2] += (double)(ec * ec * conf_mask);
                acc[3] += (double)((lse - p[5 + tcls]) * class_mask);
                acc[4] += coord_mask > 0.0f;
                acc[5] += conf_mask > 0.0f;
                acc[6] += class_mask > 0.0f;
                acc[7] += (double)t4;
                acc[8] += (tconf > 0.5f && pc > 0.3f) ? 1.0 : 0.0;
            } else {
                const float ncoord = (float)tot[4] + 1e-6f, nconf = (float)tot[5] + 1e-6f, ncls = (float)tot[6] + 1e-6f;
                float* g = a.grad + (long long)i * D;
                float dpx = -(txl - px) * coord_mask / ncoord, dpy = -(tyl - py) * coord_mask / ncoord;
                float dpw = -(twl - pw) * coord_mask / ncoord, dph = -(thl - ph) * coord_mask / ncoord;
                const float dtconf = (tconf - pc) * conf_mask / nconf;
                const float dpc = -dtconf;
                const float diou = dtconf * t4;
                if (diou != 0.0f) {
                    const float U = io.uni, I = io.inter;
                    const float dI = diou / U + diou * I / (U * U);
                    const float dUp = -diou * I / (U * U);
                    const float iw = fmaxf(io.dw, 0.0f), ih = fmaxf(io.dh, 0.0f);
                    const float ddw = (io.dw >= 0.0f) ? dI * ih : 0.0f;      // tf.maximum(d, 0.): first arg on ties
                    const float ddh = (io.dh >= 0.0f) ? dI * iw : 0.0f;
                    const float dpmaxx = (io.pmaxx <= io.tmaxx) ? ddw : 0.0f, dpmaxy = (io.pmaxy <= io.tmaxy) ? ddh : 0.0f;
                    const float dpminx = (io.pminx >= io.tminx) ? -ddw : 0.0f, dpminy = (io.pminy >= io.tminy) ? -ddh : 0.0f;
                    dpx += dpmaxx + dpminx;
                    dpy += dpmaxy + dpminy;
                    dpw += (dpmaxx - dpminx) / 2.0f + dUp * ph;
                    dph += (dpmaxy - dpminy) / 2.0f + dUp * pw;
                }
                g[0] = dpx * sx * (1.0f - sx) * a.lw;
                g[1] = dpy * sy * (1.0f - sy) * a.lw;
                g[2] = dpw * pw * a.lw;
                g[3] = dph * ph * a.lw;
                g[4] = dpc * pc * (1.0f - pc) * a.lw;
                const float cm = class_mask / ncls;
                for (int k = 0; k < a.C; ++k) {
                    const float sm = expf(p[5 + k] - mx) / se;
                    g[5 + k] = (sm - (k == tcls ? 1.0f : 0.0f)) * cm * a.lw;
                }
            }
        }
        if (pass == 0) {
            for (int k = 0; k < LOSS_NACC; ++k) red[k][tid] = acc[k];
            __syncthreads();
            for (int o = blockDim.x / 2; o > 0; o >>= 1) {
                if (tid < o)
                    for (int k = 0; k < LOSS_NACC; ++k) red[k][tid] += red[k][tid + o];
                __syncthreads();
            }
            if (tid < LOSS_NACC) tot[tid] = red[tid][0];
            __syncthreads();
            if (tid == 0) {
                const float ncoord = (float)tot[4], nconf = (float)tot[5], ncls = (float)tot[6];
                const float lxy = (float)tot[0] / (ncoord + 1e-6f) / 2.0f;
                const float lwh = (float)tot[1] / (ncoord + 1e-6f) / 2.0f;
                const float lcf = (float)tot[2] / (nconf + 1e-6f) / 2.0f;
                const float lcl = (float)tot[3] / (ncls + 1e-6f);
                a.out[0] = lxy + lwh + lcf + lcl;
                a.out[1] = lxy; a.out[2] = lwh; a.out[3] = lcf; a.out[4] = lcl;
                a.out[5] = (float)tot[8] / ((float)tot[7] + 1e-6f);
                a.out[6] = ncoord; a.out[7] = nconf;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// unmold_mask for every detection of one image (myolo_utils.py:883-912 inside MaskYOLO.decode_masks,
// model.py:1355-1389): pick the class channel, resize the mh x mw mask to the detection's clamped pixel
// window (order-1, pixel centres aligned, edge clamp -- float32, this operation order), threshold at 0.5,
// paste.  out[H][W][N] uint8 (the reference's np.stack(axis=-1) layout); lanes run along N so a wave writes
// N contiguous bytes per pixel.
// ---------------------------------------------------------------------------------------
// skimage.transform.resize(..., clip=True) clips its output to the value range of the INPUT mask.  With the zero border of
// mode='constant' that matters in exactly one case for the 0.5 threshold: a mask whose minimum is already >= 0.5 keeps its rim
// (the fade towards 0 is clipped back up to the minimum).  allhigh[n] = 1 for such a detection (its class channel).
// sel (NULL: block n reads row n): block n = slot (image n / K, slot n % K) reads row sel[n] of that image's R rows; an empty slot (sel < 0) gets 0
__global__ __launch_bounds__(256) void unmold_allhigh_kernel(const float* __restrict__ masks, const float* __restrict__ det,
                                                             int32_t* __restrict__ allhigh, int mh, int mw, int C,
                                                             const int32_t* __restrict__ sel, int K, int R)
{
    __shared__ int low;
    long long n = blockIdx.x;
    if (sel) {
        const int s = sel[blockIdx.x];
        if (s < 0 || s >= R) {
            if (threadIdx.x == 0) allhigh[blockIdx.x] = 0;
            return;
        }
        n = (long long)(blockIdx.x / K) * R + s;
    }
    if (threadIdx.x == 0) low = 0;
    __syncthreads();
    const int cls = (int)det[n * 6 + 5];
    const float* m = masks + n * mh * mw * C + cls;
    int mine = 0;
    for (int i = threadIdx.x; i < mh * mw; i += blockDim.x)
        if (!(m[(long long)i * C] >= 0.5f)) mine = 1;
    if (mine) low = 1;
    __syncthreads();
    if (threadIdx.x == 0) allhigh[blockIdx.x] = low ? 0 : 1;
}

// the clamped pixel window of one detection d = [x1, y1, x2, y2, score, class] (normalised corners)
__device__ __forceinline__ void unmold_window(const float* __restrict__ d, int H, int W, int& x1, int& y1, int& x2, int& y2)
{
    // image_shape[0] is used for x and [1] for y (myolo_utils.py:892); square images here
    x1 = min(max(0, (int)(d[0] * (float)W)), W), x2 = min(max(1, (int)(d[2] * (float)W)), W);
    y1 = min(max(0, (int)(d[1] * (float)H)), H), y2 = min(max(1, (int)(d[3] * (float)H)), H);
}

// the pasted pixel (x, y) of one detection: d its row, m0 its [mh][mw][C] mask block, allhigh its flag.  The ONE statement of the paste:
// unmold_kernel writes this byte, mask_overlap_kernel counts it.
__device__ __forceinline__ uint8_t unmold_pixel(const float* __restrict__ d, const float* __restrict__ m0, int allhigh, int x, int y, int mh,
                                                int mw, int C, int H, int W)
{
    int x1, y1, x2, y2;
    unmold_window(d, H, W, x1, y1, x2, y2);
    uint8_t v = 0;
    if (y >= y1 && y < y2 && x >= x1 && x < x2) {
        const int oh = max(1, y2 - y1), ow = max(1, x2 - x1);
        const int cls = (int)d[5];
        const float sy = (float)mh / (float)oh, sx = (float)mw / (float)ow;
        float fy = ((float)(y - y1) + 0.5f) * sy - 0.5f;
        float fx = ((float)(x - x1) + 0.5f) * sx - 0.5f;
        // skimage.transform.resize(order=1, mode='constant', cval=0) as the reference calls it (myolo_utils.py:433-447, 903):
        // samples outside the 28x28 mask read 0 (NOT the edge value), so an up-scaled mask fades to 0 over the outermost
        // half source pixel -- pinned against scikit-image 0.18.3 in tests/golden/skimage_resize_fixture.npz
        const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
        const int yb = y0 + 1, xb = x0 + 1;
        const float wy = fy - (float)y0, wx = fx - (float)x0;
        const float* m = m0 + cls;
        const bool y0in = (unsigned)y0 < (unsigned)mh, ybin = (unsigned)yb < (unsigned)mh;
        const bool x0in = (unsigned)x0 < (unsigned)mw, xbin = (unsigned)xb < (unsigned)mw;
        const float tl = (y0in && x0in) ? m[((long long)y0 * mw + x0) * C] : 0.f, tr = (y0in && xbin) ? m[((long long)y0 * mw + xb) * C] : 0.f;
        const float bl = (ybin && x0in) ? m[((long long)yb * mw + x0) * C] : 0.f, br = (ybin && xbin) ? m[((long long)yb * mw + xb) * C] : 0.f;
        const float top = tl + (tr - tl) * wx;
        const float bot = bl + (br - bl) * wx;
        v = ((top + (bot - top) * wy) >= 0.5f || allhigh) ? 1 : 0;        // clip=True: see unmold_allhigh_kernel
    }
    return v;
}

__global__ __launch_bounds__(256) void unmold_kernel(const float* __restrict__ masks, const float* __restrict__ det,
                                                     const int32_t* __restrict__ allhigh, uint8_t* __restrict__ out, int N, int mh, int mw,
                                                     int C, int H, int W)
{
    const long long total = (long long)H * W * N;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int n = (int)(i % N);
        const int pix = (int)(i / N);
        const int y = pix / W, x = pix - y * W;
        out[i] = unmold_pixel(det + (long long)n * 6, masks + (long long)n * mh * mw * C, allhigh[n], x, y, mh, mw, C, H, W);
    }
}

// ---------------------------------------------------------------------------------------
// Overlap counts for evaluation (myolo/evaluate.py): for every image b, selected detection k (row sel[b][k] of the image's R
// rows, < 0 = empty slot) and ground-truth plane t of gt [B][H][W][T] (0 / 1 bytes), the number of pixels set in both the
// PASTED mask of k -- unmold_pixel, the byte unmold_kernel would write -- and plane t; plus each pasted mask's and each plane's
// own pixel count and the paste window.  No full-size mask is written.
// One workgroup = OV_GROUPS consecutive groups of 64 pixels (row-major) of one image, a wave per group: a ballot turns each of
// the K paste decisions and each of the T ground-truth bytes of the group's 64 pixels into one 64-bit word, the K x T
// intersections are popcounts of ANDs spread over the lanes (pair q = lane + 64 j; the words go through LDS), accumulated in
// registers over the wave's groups, summed over the four waves and added into the zeroed outputs with integer atomics
// (integer sums: the order cannot matter).  A group's 64 T ground-truth bytes are contiguous and 64-byte aligned relative to
// the buffer: 16-byte loads, transposed through LDS (gt_vec: the buffer itself is 16-byte aligned; the last, partial group
// of an image reads bytes).
// ---------------------------------------------------------------------------------------
#define OV_MAXK 16
#define OV_MAXT 32
#define OV_GROUPS 16
#define OV_PAIRS ((OV_MAXK * OV_MAXT) / 64)

__global__ __launch_bounds__(256) void mask_overlap_kernel(const float* __restrict__ masks, const float* __restrict__ det,
                                                           const int32_t* __restrict__ sel, const int32_t* __restrict__ allhigh,
                                                           const uint8_t* __restrict__ gt, int32_t* __restrict__ inter,
                                                           int32_t* __restrict__ area_pred, int32_t* __restrict__ area_gt,
                                                           int32_t* __restrict__ win, int R, int K, int T, int mh, int mw, int C, int H, int W,
                                                           int gt_vec)
{
    __shared__ uint4 gtL[4][OV_MAXT * 4];                          // one group's 64 x T bytes per wave
    __shared__ unsigned long long pwL[4][OV_MAXK], gwL[4][OV_MAXT];
    __shared__ int red[4][OV_PAIRS + 2][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y;
    const int P = H * W, ngroups = (P + 63) / 64, KT = K * T;
    int acc[OV_PAIRS], accP = 0, accG = 0;
#pragma unroll
    for (int j = 0; j < OV_PAIRS; ++j) acc[j] = 0;

    for (int it = 0; it < OV_GROUPS / 4; ++it) {
        const int g = blockIdx.x * OV_GROUPS + it * 4 + wave;
        const bool live = g < ngroups;                             // the same for the whole wave
        const int p = g * 64 + lane;
        const bool inimg = live && p < P;
        if (live) {
            const long long byte0 = ((long long)b * P + (long long)g * 64) * T;
            if (gt_vec && g * 64 + 64 <= P) {
                const uint4* src = (const uint4*)(gt + byte0);
                for (int j = lane; j < 4 * T; j += 64) gtL[wave][j] = src[j];
            } else {
                uint8_t* dst = (uint8_t*)gtL[wave] + lane * T;
                for (int t = 0; t < T; ++t) dst[t] = inimg ? gt[byte0 + (long long)lane * T + t] : (uint8_t)0;
            }
        }
        __syncthreads();
        if (live) {
            const uint8_t* mine = (const uint8_t*)gtL[wave] + lane * T;
            for (int t = 0; t < T; ++t) {
                const unsigned long long w = __ballot(mine[t] != 0);
                if (lane == 0) gwL[wave][t] = w;
            }
            const int y = p / W, x = p - y * W;
            for (int k = 0; k < K; ++k) {
                const int s = sel[b * K + k];
                int v = 0;
                if (s >= 0 && s < R && inimg) {
                    const long long row = (long long)b * R + s;
                    v = unmold_pixel(det + row * 6, masks + row * mh * mw * C, allhigh[b * K + k], x, y, mh, mw, C, H, W);
                }
                const unsigned long long w = __ballot(v);
                if (lane == 0) pwL[wave][k] = w;
            }
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int j = 0; j < OV_PAIRS; ++j) {
                const int q = lane + 64 * j;
                if (q < KT) acc[j] += __popcll(pwL[wave][q / T] & gwL[wave][q % T]);
            }
            if (lane < K) accP += __popcll(pwL[wave][lane]);
            if (lane < T) accG += __popcll(gwL[wave][lane]);
        }
    }
#pragma unroll
    for (int j = 0; j < OV_PAIRS; ++j) red[wave][j][lane] = acc[j];
    red[wave][OV_PAIRS][lane] = accP;
    red[wave][OV_PAIRS + 1][lane] = accG;
    __syncthreads();
    for (int q = tid; q < KT; q += 256) {
        const int s = red[0][q >> 6][q & 63] + red[1][q >> 6][q & 63] + red[2][q >> 6][q & 63] + red[3][q >> 6][q & 63];
        if (s) atomicAdd(inter + (long long)b * KT + q, s);
    }
    if (tid < K) {
        const int s = red[0][OV_PAIRS][tid] + red[1][OV_PAIRS][tid] + red[2][OV_PAIRS][tid] + red[3][OV_PAIRS][tid];
        if (s) atomicAdd(area_pred + (long long)b * K + tid, s);
    }
    if (tid < T) {
        const int s = red[0][OV_PAIRS + 1][tid] + red[1][OV_PAIRS + 1][tid] + red[2][OV_PAIRS + 1][tid] + red[3][OV_PAIRS + 1][tid];
        if (s) atomicAdd(area_gt + (long long)b * T + tid, s);
    }
    if (blockIdx.x == 0 && tid < K) {
        const int s = sel[b * K + tid];
        int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        if (s >= 0 && s < R) unmold_window(det + ((long long)b * R + s) * 6, H, W, x1, y1, x2, y2);
        int32_t* o = win + ((long long)b * K + tid) * 4;
        o[0] = x1, o[1] = y1, o[2] = x2, o[3] = y2;
    }
}

// ---------------------------------------------------------------------------------------
// Run-length form of the pasted masks (myolo/rle.py): for every image b (its own output frame h x w, frames [B][2]) and
// selected detection k, the BOUNDARIES of the pasted mask in COCO's column-major pixel order p = x * h + y: every p in [0, h * w) whose pixel
// differs from pixel p - 1 (pixel -1 = 0).  A pixel is unmold_pixel -- the byte unmold_kernel would write -- so the runs are the dense paste's
// by construction; no full-size mask is written.
// Outside the paste window every pixel is 0, so a boundary has p or p - 1 inside it.  One wave owns one window column x and walks the rows
// ya .. yb (rle_column_rows) 64 at a time: a ballot of the 64 pixels, XOR with itself shifted by one (the carried last pixel of the previous
// group coming in at bit 0) gives the boundaries, a popcount their number, the popcount below a lane its boundary's rank.  The pixel before a
// column's first row is pixel p - 1: the last row of the column to the left when the window starts at row 0 (a run goes on across the column
// joint without a boundary), 0 otherwise.  rle_columns_kernel<false> leaves the number of boundaries of column x of slot s in
// cols [s][max_w]; rle_scan_columns_kernel scans every slot's row in place and leaves the slot's total in run_off [s], rle_scan_slots_kernel
// scans those; rle_columns_kernel<true> walks again and stores each boundary at run_off[s] + cols[s][x] + rank -- when that lies below cap.
// Integer work only: bit-identical from run to run.
// ---------------------------------------------------------------------------------------
// the rows ya .. yb (both included) of window column x that the column's wave owns; row H stands for row 0 of column x + 1, the pixel behind the
// column's last one.  That pixel belongs to column x + 1's wave when the window has that column and starts at row 0, and to nobody when it is
// pixel H * W.  false: x is no column of the window (or the window holds no pixel).
__device__ __forceinline__ bool rle_column_rows(const float* __restrict__ d, int H, int W, int x, int& ya, int& yb)
{
    int x1, y1, x2, y2;
    unmold_window(d, H, W, x1, y1, x2, y2);
    if (x < x1 || x >= x2 || y1 >= y2) return false;
    ya = y1, yb = y2;
    if (y2 == H && ((y1 == 0 && x + 1 < x2) || x + 1 == W)) yb = H - 1;
    return true;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void rle_columns_kernel(const float* __restrict__ masks, const float* __restrict__ det,
                                                          const int32_t* __restrict__ sel, const int32_t* __restrict__ allhigh,
                                                          const int32_t* __restrict__ frames, int32_t* __restrict__ cols,
                                                          const int32_t* __restrict__ run_off, uint32_t* __restrict__ bounds, long long cap,
                                                          int R, int K, int mh, int mw, int C, int max_w)
{
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 4 + (threadIdx.x >> 6);            // one column per wave: everything below is uniform over the wave
    const int slot = blockIdx.y, b = slot / K;
    if (x >= max_w) return;
    const int s = sel[slot];
    const int H = frames[2 * b], W = frames[2 * b + 1];
    const long long row = (long long)b * R + max(s, 0);
    const float* d = det + row * 6;
    int ya = 0, yb = -1;
    if (!(s >= 0 && s < R && x < W && rle_column_rows(d, H, W, x, ya, yb))) {
        if (!WRITE && lane == 0) cols[(long long)slot * max_w + x] = 0;
        return;
    }
    const float* m0 = masks + row * mh * mw * C;
    const int ah = allhigh[slot];
    unsigned long long carry = (ya == 0 && x > 0) ? unmold_pixel(d, m0, ah, x - 1, H - 1, mh, mw, C, H, W) : 0;
    const long long base = WRITE ? (long long)run_off[slot] + cols[(long long)slot * max_w + x] : 0;
    int n = 0;
    for (int y0 = ya; y0 <= yb; y0 += 64) {
        const int y = y0 + lane;
        const bool in = y <= yb;
        int v = 0;
        if (in) v = (y < H) ? unmold_pixel(d, m0, ah, x, y, mh, mw, C, H, W) : unmold_pixel(d, m0, ah, x + 1, 0, mh, mw, C, H, W);
        const unsigned long long bits = __ballot(v), valid = __ballot(in);
        const unsigned long long bnd = (bits ^ ((bits << 1) | carry)) & valid;
        carry = bits >> 63;
        if (WRITE && ((bnd >> lane) & 1ull)) {
            const long long at = base + n + __popcll(bnd & ((1ull << lane) - 1ull));
            if (at < cap) bounds[at] = (uint32_t)(x * H + y);
        }
        n += __popcll(bnd);
    }
    if (!WRITE && lane == 0) cols[(long long)slot * max_w + x] = n;
}

// a [0, n) -> its exclusive prefix sums, in place, by one workgroup of 256; -> the total (in every thread)
__device__ __forceinline__ int rle_scan_in_place(int32_t* __restrict__ a, int n)
{
    __shared__ int wsum[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const int v = i < n ? a[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int off = carry;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (i < n) a[i] = off + inc - v;
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    return carry;
}

__global__ __launch_bounds__(256) void rle_scan_columns_kernel(int32_t* __restrict__ cols, int32_t* __restrict__ run_off, int max_w)
{
    const int total = rle_scan_in_place(cols + (long long)blockIdx.x * max_w, max_w);
    if (threadIdx.x == 0) run_off[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void rle_scan_slots_kernel(int32_t* __restrict__ run_off, int nslots)
{
    const int total = rle_scan_in_place(run_off, nslots);
    if (threadIdx.x == 0) run_off[nslots] = total;
}

// ---------------------------------------------------------------------------------------
// Outlines of the pasted masks (myolo/contour.py is the statement of the contract): for every image b (its own frame) and
// selected detection k, the closed loops of the mask's boundary as vertex lists in lattice corner coordinates.  A pixel is unmold_pixel, so the
// outline is contour.trace of the dense paste by construction; no dense mask is written, and everything behind unmold_pixel is integer work.
//
// The four pixels round corner (X, Y) -- a b in row Y - 1 (columns X - 1, X), c d in row Y -- decide what starts there: the edge leaving east
// exists when d & ~b, south c & ~d, west a & ~c, north b & ~a, and the edge ARRIVING with a direction when c & ~a, a & ~b, b & ~d, d & ~c.  A
// leaving edge is a vertex edge unless the edge arriving with its own direction exists (a straight joint); a corner holds 0, 1 or -- between two
// pixels that touch diagonally -- 2 of them.  Outside the paste window every pixel is 0, so only the window's corners x1 .. x2, y1 .. y2 matter.
//  1. contour_rows_kernel<false>: one wave per lattice row, 64 corners at a time: ballots of the rows Y - 1 and Y, shifted by one for the
//     columns X - 1 (the last bits of the previous group carried in), four bitwise expressions, popcounts.  rows [slot][Y] = vertex edges of the row.
//  2. rle_scan_columns_kernel / rle_scan_slots_kernel: the rows of a slot and the slots, exclusive, vert_off [nslots + 1].
//  3. contour_rows_kernel<true>: the same walk stores the keys (Y << 33 | X << 2 | dir) compacted: ascending within a slot.
//  4. contour_link_kernel: one lane per vertex edge walks along its direction (two pixels per step decide right turn / straight / left turn)
//     to the corner where the direction changes, and finds that vertex edge's index by binary search in the slot's keys: succ.  After
//     CT_SOLO steps of its own a stretch is walked by the whole wave, 64 steps at a time (one lane walking a window's side of 416 steps was
//     two thirds of the entry's time on filled windows).
//  5. contour_rank_kernel: ONE workgroup per slot (a loop never leaves its slot, so __syncthreads() is the only barrier): pointer jumping over
//     double buffers gives every vertex the smallest index of its loop; with every cycle cut in front of that head a second set of rounds gives
//     the distance to the loop's end; the heads' lengths and flags are scanned in index (= key) order for the loop offsets and ordinals, and
//     every vertex is stored at vert_off[slot] + offset of its loop + its rank.
// Steps 3-5 do nothing when vert_off[nslots] > cap (the caller grows its buffers and calls again); nothing is written at or beyond cap.
// ---------------------------------------------------------------------------------------
#define CT_LINK_BLOCKS 8

template <bool WRITE>
__global__ __launch_bounds__(256) void contour_rows_kernel(const float* __restrict__ masks, const float* __restrict__ det,
                                                           const int32_t* __restrict__ sel, const int32_t* __restrict__ allhigh,
                                                           const int32_t* __restrict__ frames, int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ vert_off, unsigned long long* __restrict__ keys,
                                                           long long cap, int nslots, int R, int K, int mh, int mw, int C, int max_rows)
{
    const int lane = threadIdx.x & 63;
    const int Y = blockIdx.x * 4 + (threadIdx.x >> 6);            // one lattice row per wave: everything below is uniform over the wave
    const int slot = blockIdx.y, b = slot / K;
    if (Y >= max_rows) return;
    if (WRITE && (long long)vert_off[nslots] > cap) return;
    const int s = sel[slot];
    const int H = frames[2 * b], W = frames[2 * b + 1];
    const long long row = (long long)b * R + max(s, 0);
    const float* d = det + row * 6;
    int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    if (s >= 0 && s < R) unmold_window(d, H, W, x1, y1, x2, y2);
    if (!(s >= 0 && s < R && x1 < x2 && y1 < y2 && Y >= y1 && Y <= y2)) {
        if (!WRITE && lane == 0) rows[(long long)slot * max_rows + Y] = 0;
        return;
    }
    const float* m0 = masks + row * mh * mw * C;
    const int ah = allhigh[slot];
    const long long base = WRITE ? (long long)vert_off[slot] + rows[(long long)slot * max_rows + Y] : 0;
    unsigned long long carry_t = 0, carry_b = 0;                   // the pixels of column x1 - 1: outside the window
    int n = 0;
    for (int x0 = x1; x0 <= x2; x0 += 64) {
        const int X = x0 + lane;
        int top = 0, bot = 0;
        if (X <= x2) {                                             // (column x2 and the rows y1 - 1, y2 lie outside the window: unmold_pixel gives 0)
            top = unmold_pixel(d, m0, ah, X, Y - 1, mh, mw, C, H, W);
            bot = unmold_pixel(d, m0, ah, X, Y, mh, mw, C, H, W);
        }
        const unsigned long long pb = __ballot(top), pd = __ballot(bot);
        const unsigned long long pa = (pb << 1) | carry_t, pc = (pd << 1) | carry_b;
        carry_t = pb >> 63, carry_b = pd >> 63;
        const unsigned long long vE = (pd & ~pb) & ~(pc & ~pa), vS = (pc & ~pd) & ~(pa & ~pb);
        const unsigned long long vW = (pa & ~pc) & ~(pb & ~pd), vN = (pb & ~pa) & ~(pd & ~pc);
        if (WRITE) {
            const unsigned long long below = (1ull << lane) - 1ull;
            long long at = base + n + __popcll(vE & below) + __popcll(vS & below) + __popcll(vW & below) + __popcll(vN & below);
            const unsigned long long v[4] = {vE, vS, vW, vN};
#pragma unroll
            for (int dir = 0; dir < 4; ++dir)
                if ((v[dir] >> lane) & 1ull) {
                    if (at < cap) keys[at] = ((unsigned long long)Y << 33) | ((unsigned long long)X << 2) | (unsigned long long)dir;
                    ++at;
                }
        }
        n += __popcll(vE) + __popcll(vS) + __popcll(vW) + __popcll(vN);
    }
    if (!WRITE && lane == 0) rows[(long long)slot * max_rows + Y] = n;
}

#define CT_SOLO 8
__device__ __forceinline__ int ct_dx(int dir) { return dir == 0 ? 1 : (dir == 2 ? -1 : 0); }
__device__ __forceinline__ int ct_dy(int dir) { return dir == 1 ? 1 : (dir == 3 ? -1 : 0); }
// corner (X, Y) reached with direction dir along an edge: the direction of the edge that goes on from it when that is a turn, -1 when it goes
// straight on.  Two pixels ahead of the corner decide: the one on the right of travel (the inside so far) clear -- a right turn; else the one on
// the left set -- a left turn.
__device__ __forceinline__ int ct_turn(const float* __restrict__ d, const float* __restrict__ m0, int ah, int X, int Y, int dir, int mh, int mw,
                                       int C, int H, int W)
{
    const int rx = (dir == 1 || dir == 2) ? -1 : 0, ry = (dir == 2 || dir == 3) ? -1 : 0;
    const int lx = (dir == 2 || dir == 3) ? -1 : 0, ly = (dir == 0 || dir == 3) ? -1 : 0;
    if (!unmold_pixel(d, m0, ah, X + rx, Y + ry, mh, mw, C, H, W)) return (dir + 1) & 3;
    if (unmold_pixel(d, m0, ah, X + lx, Y + ly, mh, mw, C, H, W)) return (dir + 3) & 3;
    return -1;
}

__global__ __launch_bounds__(256) void contour_link_kernel(const float* __restrict__ masks, const float* __restrict__ det,
                                                           const int32_t* __restrict__ sel, const int32_t* __restrict__ allhigh,
                                                           const int32_t* __restrict__ frames, const int32_t* __restrict__ vert_off,
                                                           const unsigned long long* __restrict__ keys, int32_t* __restrict__ succ,
                                                           long long cap, int nslots, int R, int K, int mh, int mw, int C)
{
    const int slot = blockIdx.y, b = slot / K;
    if ((long long)vert_off[nslots] > cap) return;
    const int base = vert_off[slot], V = vert_off[slot + 1] - base;
    const int s = sel[slot];
    if (V <= 0 || s < 0 || s >= R) return;
    const int H = frames[2 * b], W = frames[2 * b + 1];
    const long long row = (long long)b * R + s;
    const float* d = det + row * 6;
    const float* m0 = masks + row * mh * mw * C;
    const int ah = allhigh[slot];
    const int lane = threadIdx.x & 63;
    const int groups = ((H > W ? H : W) + 63) / 64 + 1;             // no straight stretch is longer than a side of the frame
    // 64 vertex edges per wave at a time (i0 is uniform over the wave): a lane walks its own edge CT_SOLO steps -- a ragged outline's stretches
    // end there -- and the wave then takes the unfinished ones in turn, 64 steps at a time, the first turn found by a ballot
    for (int i0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; i0 < V; i0 += CT_LINK_BLOCKS * 256) {
        const int i = i0 + lane;
        const bool mine = i < V;
        const unsigned long long key = mine ? keys[base + i] : 0ull;
        const int dir = (int)(key & 3ull);
        int X = (int)((key >> 2) & 0x7fffffffull), Y = (int)(key >> 33);
        int nd = -1;
        if (mine) {
            const int dx = ct_dx(dir), dy = ct_dy(dir);
            for (int step = 0; step < CT_SOLO && nd < 0; ++step) {
                X += dx, Y += dy;
                nd = ct_turn(d, m0, ah, X, Y, dir, mh, mw, C, H, W);
            }
        }
        unsigned long long pending = __ballot(mine && nd < 0);
        while (pending) {
            const int src = __ffsll((long long)pending) - 1;
            pending &= pending - 1ull;
            const int sdir = __shfl(dir, src), sx = __shfl(X, src), sy = __shfl(Y, src);
            const int dx = ct_dx(sdir), dy = ct_dy(sdir);
            for (int g = 0; g < groups; ++g) {
                const int k = g * 64 + lane + 1;                   // (a lane beyond the turn reads pixels that may lie outside the frame: they are 0)
                const int t = ct_turn(d, m0, ah, sx + k * dx, sy + k * dy, sdir, mh, mw, C, H, W);
                const unsigned long long turned = __ballot(t >= 0);
                if (turned) {
                    const int first = __ffsll((long long)turned) - 1;
                    const int tn = __shfl(t, first);
                    if (lane == src) X = sx + (g * 64 + first + 1) * dx, Y = sy + (g * 64 + first + 1) * dy, nd = tn;
                    break;
                }
            }
        }
        if (!mine) continue;
        int found = i;                                             // (a key that is not there cannot happen; the link then stays inside the slot)
        if (nd >= 0) {
            const unsigned long long want = ((unsigned long long)Y << 33) | ((unsigned long long)X << 2) | (unsigned long long)nd;
            int lo = 0, hi = V - 1;
            while (lo <= hi) {
                const int mid = (lo + hi) >> 1;
                const unsigned long long k = keys[base + mid];
                if (k == want) { found = mid; break; }
                if (k < want) lo = mid + 1; else hi = mid - 1;
            }
        }
        succ[base + i] = found;
    }
}

// buffers of cap words each, indexed vert_off[slot] + i; the values are indices inside the slot.  No __restrict__: they are exchanged between
// the waves of the workgroup from round to round.
__global__ __launch_bounds__(256) void contour_rank_kernel(const int32_t* vert_off, const unsigned long long* keys, const int32_t* succ,
                                                           int32_t* m0, int32_t* m1, int32_t* n0, int32_t* n1, int32_t* d0, int32_t* d1,
                                                           int32_t* s0, int32_t* s1, int32_t* verts, int32_t* loop_id, long long cap, int nslots)
{
    if ((long long)vert_off[nslots] > cap) return;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int base = vert_off[slot], V = vert_off[slot + 1] - base;
    if (V <= 0) return;
    keys += base, succ += base, m0 += base, m1 += base, n0 += base, n1 += base, d0 += base, d1 += base, s0 += base, s1 += base;
    int rounds = 0;
    while ((1ll << rounds) < V) ++rounds;
    // every vertex's loop head: the smallest index on its cycle
    for (int i = tid; i < V; i += 256) m0[i] = i, n0[i] = succ[i];
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
        for (int i = tid; i < V; i += 256) {
            const int j = n0[i];
            m1[i] = min(m0[i], m0[j]);
            n1[i] = n0[j];
        }
        __syncthreads();
        int32_t* t = m0; m0 = m1; m1 = t;
        t = n0; n0 = n1; n1 = t;
    }
    // the distance to the end of the loop, the cycle cut in front of its head (m0 is final and stays)
    for (int i = tid; i < V; i += 256) {
        const int j = succ[i];
        const bool last = j == m0[i];
        n0[i] = last ? -1 : j;
        d0[i] = last ? 0 : 1;
    }
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
        for (int i = tid; i < V; i += 256) {
            const int j = n0[i];
            d1[i] = j < 0 ? d0[i] : d0[i] + d0[j];
            n1[i] = j < 0 ? -1 : n0[j];
        }
        __syncthreads();
        int32_t* t = d0; d0 = d1; d1 = t;
        t = n0; n0 = n1; n1 = t;
    }
    // loop offsets and ordinals: the heads in index order
    for (int i = tid; i < V; i += 256) {
        const bool head = m0[i] == i;
        s0[i] = head ? d0[i] + 1 : 0;
        s1[i] = head ? 1 : 0;
    }
    __syncthreads();
    rle_scan_in_place(s0, V);
    rle_scan_in_place(s1, V);
    for (int i = tid; i < V; i += 256) {
        const int h = m0[i];
        const int at = s0[h] + (d0[h] - d0[i]);
        if (at >= 0 && at < V && (long long)base + at < cap) {
            const unsigned long long key = keys[i];
            verts[2 * ((long long)base + at)] = (int)((key >> 2) & 0x7fffffffull);
            verts[2 * ((long long)base + at) + 1] = (int)(key >> 33);
            loop_id[(long long)base + at] = s1[h];
        }
    }
}

// ---------------------------------------------------------------------------------------
// Overlay of the selected detections on the uploaded image bytes (myolo/render.py render_instances is the statement of the picture, DESIGN.md
// section 16): for every image b of a packed batch (desc [B][3] = byte offset, h, w, the pack_images layout) the three layers of the host
// renderer -- blend every pasted mask into the canvas, draw the one-pixel outline of every mask, blend the dashed ring of every paste window --
// each over the slots k = 0 .. K-1 in order, written as uint8 at the image's own offset.  A mask pixel is unmold_pixel, so the picture is the
// host render of the dense paste byte for byte; no dense mask is written.
// One workgroup = one RN_TW x RN_TH tile of one image.  It first leaves in LDS, for every pixel of the tile and of a one-pixel halo around it,
// the word whose bit k says that slot k's pasted mask holds the pixel (0 outside the frame: the zero padding the outline is defined on); only
// the slots whose window meets the haloed tile are evaluated, a test that is the same for the whole workgroup.  Then every thread takes four
// pixels in a row: its membership word and those of the four neighbours come from LDS, the blend runs in double with the product and the sum
// as two roundings (no fused multiply-add: this file is compiled with -ffp-contract=off, and the intrinsics say so again) and truncates into
// the canvas as numpy's store into a uint32 array does.  Four pixels are 12 bytes: loaded and stored as three dwords when the row's first
// byte is 4-byte aligned (every row of an image whose width is a multiple of 4 in a batch of such images), as bytes otherwise.
// ---------------------------------------------------------------------------------------
#define RN_TW 128
#define RN_TH 8
#define RN_PITCH (RN_TW + 4)
#define RN_HALO_PIXELS ((RN_TW + 2) * (RN_TH + 2))
#define RN_FILL ((RN_HALO_PIXELS + 255) / 256)
#define RN_BLEND 1
#define RN_OUTLINE 2
#define RN_BOX 4

__global__ __launch_bounds__(256) void render_instances_kernel(const uint8_t* __restrict__ images, uint8_t* __restrict__ out,
                                                               const int64_t* __restrict__ desc, const float* __restrict__ masks,
                                                               const float* __restrict__ det, const int32_t* __restrict__ sel,
                                                               const int32_t* __restrict__ allhigh, const double* __restrict__ colors,
                                                               double alpha, double box_alpha, int flags, int R, int K, int mh, int mw, int C)
{
    __shared__ unsigned short memb[RN_TH + 2][RN_PITCH];
    __shared__ int winL[OV_MAXK][4];                               // [x1, y1, x2, y2) of the slot's paste; x2 = 0 for a slot that draws nothing
    __shared__ double blendL[OV_MAXK][3], boxL[OV_MAXK][3];        // (alpha * colour) * 255 of layer 1 and of layer 3
    __shared__ unsigned lineL[OV_MAXK][3];                         // uint32(colour * 255) of layer 2
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long off = desc[3 * b];
    const int H = (int)desc[3 * b + 1], W = (int)desc[3 * b + 2];
    const int tiles_x = (W + RN_TW - 1) / RN_TW, tiles_y = (H + RN_TH - 1) / RN_TH;
    if ((long long)blockIdx.x >= (long long)tiles_x * tiles_y) return;                  // the grid is the largest image's: uniform over the workgroup
    const int tx0 = (int)(blockIdx.x % tiles_x) * RN_TW, ty0 = (int)(blockIdx.x / tiles_x) * RN_TH;

    if (tid < K) {
        const int s = sel[b * K + tid];
        int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        if (s >= 0 && s < R) unmold_window(det + ((long long)b * R + s) * 6, H, W, x1, y1, x2, y2);
        if (x2 <= x1 || y2 <= y1) x1 = y1 = x2 = y2 = 0;
        winL[tid][0] = x1, winL[tid][1] = y1, winL[tid][2] = x2, winL[tid][3] = y2;
    }
    if (tid < 3 * K) {
        const int k = tid / 3, c = tid - 3 * k;
        const double col = colors[((long long)b * K + k) * 3 + c];
        blendL[k][c] = __dmul_rn(__dmul_rn(alpha, col), 255.0);
        boxL[k][c] = __dmul_rn(__dmul_rn(box_alpha, col), 255.0);
        lineL[k][c] = (unsigned)__dmul_rn(col, 255.0);
    }
    __syncthreads();

    // the membership words of the haloed tile
    unsigned word[RN_FILL];
#pragma unroll
    for (int j = 0; j < RN_FILL; ++j) word[j] = 0;
    for (int k = 0; k < K; ++k) {
        const int x1 = winL[k][0], y1 = winL[k][1], x2 = winL[k][2], y2 = winL[k][3];
        // an empty slot or window (sel may be -1: nothing below may be read), or a window clear of the haloed tile
        if (x2 <= x1 || x2 <= tx0 - 1 || x1 >= tx0 + RN_TW + 1 || y2 <= ty0 - 1 || y1 >= ty0 + RN_TH + 1) continue;
        const long long row = (long long)b * R + sel[b * K + k];
        const float* d = det + row * 6;
        const float* m0 = masks + row * mh * mw * C;
        const int ah = allhigh[b * K + k];
#pragma unroll
        for (int j = 0; j < RN_FILL; ++j) {
            const int p = tid + 256 * j;
            const int py = p / (RN_TW + 2), px = p - py * (RN_TW + 2);
            const int x = tx0 - 1 + px, y = ty0 - 1 + py;
            if (p < RN_HALO_PIXELS && x >= 0 && x < W && y >= 0 && y < H)
                word[j] |= (unsigned)unmold_pixel(d, m0, ah, x, y, mh, mw, C, H, W) << k;
        }
    }
#pragma unroll
    for (int j = 0; j < RN_FILL; ++j) {
        const int p = tid + 256 * j;
        const int py = p / (RN_TW + 2), px = p - py * (RN_TW + 2);
        if (p < RN_HALO_PIXELS) memb[py][px] = (unsigned short)word[j];
    }
    __syncthreads();

    // four pixels of one row per thread
    const int ly = tid / (RN_TW / 4), lx = (tid - ly * (RN_TW / 4)) * 4;
    const int y = ty0 + ly, xa = tx0 + lx;
    if (y >= H || xa >= W) return;
    const int npix = min(4, W - xa);
    const long long at = off + ((long long)y * W + xa) * 3;
    const uint8_t* src = images + at;
    uint8_t* dst = out + at;
    const bool wide = npix == 4 && ((((uintptr_t)src) | ((uintptr_t)dst)) & 3) == 0;
    unsigned px3[3];                                               // the 12 bytes, little-endian
    if (wide) {
        px3[0] = ((const unsigned*)src)[0], px3[1] = ((const unsigned*)src)[1], px3[2] = ((const unsigned*)src)[2];
    } else {
        px3[0] = px3[1] = px3[2] = 0;
        for (int i = 0; i < 3 * npix; ++i) px3[i >> 2] |= (unsigned)src[i] << (8 * (i & 3));
    }
    const double keep1 = 1.0 - alpha, keep3 = 1.0 - box_alpha;
    unsigned res[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned cv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) cv[c] = (px3[(3 * i + c) >> 2] >> (8 * ((3 * i + c) & 3))) & 255u;
        if (i < npix) {
            const int x = xa + i;
            const unsigned m = memb[ly + 1][lx + i + 1];
            if (flags & RN_BLEND)
                for (unsigned rest = m; rest; rest &= rest - 1) {
                    const int k = __ffs(rest) - 1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) cv[c] = (unsigned)__dadd_rn(__dmul_rn((double)cv[c], keep1), blendL[k][c]);
                }
            if (flags & RN_OUTLINE) {
                // on the outline of slot k: set, and one of the four neighbours (0 beyond the frame) is not.  The slots are drawn in order, so the
                // last one shows.
                const unsigned edge = m & ~(memb[ly][lx + i + 1] & memb[ly + 2][lx + i + 1] & memb[ly + 1][lx + i] & memb[ly + 1][lx + i + 2]);
                if (edge) {
                    const int k = 31 - __clz(edge);
                    cv[0] = lineL[k][0], cv[1] = lineL[k][1], cv[2] = lineL[k][2];
                }
            }
            if (flags & RN_BOX)
                for (int k = 0; k < K; ++k) {
                    const int x1 = winL[k][0], y1 = winL[k][1], x2 = winL[k][2], y2 = winL[k][3];
                    if (x < x1 || x >= x2 || y < y1 || y >= y2) continue;
                    const bool band = y - y1 < 2 || y2 - 1 - y < 2;                    // the top or the bottom band of the ring
                    if (!band && !(x - x1 < 2 || x2 - 1 - x < 2)) continue;
                    if ((((band ? x - x1 : y - y1) / 6) & 1) != 0) continue;           // the gaps of the dashes
#pragma unroll
                    for (int c = 0; c < 3; ++c) cv[c] = (unsigned)__dadd_rn(__dmul_rn((double)cv[c], keep3), boxL[k][c]);
                }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) res[(3 * i + c) >> 2] |= (cv[c] & 255u) << (8 * ((3 * i + c) & 3));
    }
    if (wide) {
        ((unsigned*)dst)[0] = res[0], ((unsigned*)dst)[1] = res[1], ((unsigned*)dst)[2] = res[2];
    } else {
        for (int i = 0; i < 3 * npix; ++i) dst[i] = (uint8_t)(res[i >> 2] >> (8 * (i & 3)));
    }
}

// ---------------------------------------------------------------------------------------
// Measurements of the pasted masks (myolo/measure.py measure_dense is the statement of the record): for every image b (its
// own frame h x w) and selected detection k, MYOLO_MEASURE_WORDS exact integer sums over the mask: area, the area no earlier slot of the image
// covers, the first and second raw moments, the perimeter, the 2 x 2 blocks and the tight box.  A pixel is unmold_pixel, so the sums are those of
// the dense paste by construction; no dense mask is written, and everything behind unmold_pixel is integer work.
// A wave owns one tile of MS_TW columns x MS_TH rows of one image, a lane per column, and walks the image's slots IN ORDER; a slot whose window,
// grown by one column to the left and one row upwards, misses the tile is skipped, so the work follows the windows and not K x the frame.  The
// lane evaluates the window's rows of its column into one 32-bit word (bit i = row ty0 + i) and the pixel above the tile; lanes 0 .. 32 also
// evaluate the column left of the tile and the corner, which a ballot turns into lane 0's left neighbour.  From there on it is bit work:
//   area / visible     popc(w), popc(w & ~covered) with `covered` the OR of the words of the earlier slots
//   moments            with i the bit index and l the lane, the wave sums of popc, sum i, sum i^2, l * popc, l^2 * popc, l * sum i (sums over the
//                      set bits from popcounts under the masks of the index's binary digits) are shifted to (tx0 + l, ty0 + i) in 64 bits
//   perimeter          every unit edge between a set pixel and a clear one (or the frame's outside) belongs to the tile of its lower / right
//                      pixel: the transitions against the word shifted down by one row, and against the left neighbour's word; the frame's
//                      bottom and right edges belong to the last row / column
//   quads              a 2 x 2 block belongs to its bottom-right pixel: w & left & both shifted down by one row
// The partial sums of a slot are reduced over the wave, added into the workgroup's record in LDS (integer atomics), and every workgroup adds its
// non-trivial words into out with one 64-bit integer atomic each (add, min for x1 / y1, max for x2 / y2): integer sums, the same bits every run.
// measure_init_kernel writes every word of out first (zeros, the identity of min in x1 / y1); measure_finish_kernel zeroes the box of an empty mask.
// ---------------------------------------------------------------------------------------
#define MS_MAXK 128
#define MS_TW 64
#define MS_TH 32
#define MS_NONE 0xFFFFFFFFFFFFFFFFull                             // x1 / y1 before any pixel: the identity of min

__device__ __forceinline__ unsigned ms_wave_sum(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ unsigned ms_wave_or(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// sum of i and of i * i over the set bits i of w: i = sum_j d_j 2^j, so sum i = sum_j 2^j popc(w & D_j) and
// sum i^2 = sum_j 4^j popc(w & D_j) + sum_{j<k} 2^(j+k+1) popc(w & D_j & D_k), D_j = the bit positions whose digit j is 1
__device__ __forceinline__ void ms_bit_index_sums(unsigned w, unsigned& s1, unsigned& s2)
{
    const unsigned D[5] = {0xAAAAAAAAu, 0xCCCCCCCCu, 0xF0F0F0F0u, 0xFF00FF00u, 0xFFFF0000u};
    s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const unsigned c = __popc(w & D[j]);
        s1 += c << j;
        s2 += c << (2 * j);
#pragma unroll
        for (int k = j + 1; k < 5; ++k) s2 += (unsigned)__popc(w & D[j] & D[k]) << (j + k + 1);
    }
}

__global__ __launch_bounds__(256) void measure_init_kernel(unsigned long long* __restrict__ out, int nslots)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nslots * MYOLO_MEASURE_WORDS) return;
    const int word = i % MYOLO_MEASURE_WORDS;
    out[i] = (word == 9 || word == 10) ? MS_NONE : 0ull;
}

__global__ __launch_bounds__(256) void measure_finish_kernel(unsigned long long* __restrict__ out, int nslots)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    unsigned long long* o = out + (long long)s * MYOLO_MEASURE_WORDS;
    if (o[0] == 0ull) o[9] = o[10] = 0ull;                         // (x2, y2 are still the zeros of the init)
}

__global__ __launch_bounds__(256) void measure_masks_kernel(const float* __restrict__ masks, const float* __restrict__ det,
                                                            const int32_t* __restrict__ sel, const int32_t* __restrict__ allhigh,
                                                            const int32_t* __restrict__ frames, unsigned long long* __restrict__ out, int R,
                                                            int K, int mh, int mw, int C)
{
    __shared__ int winL[MS_MAXK][4];                               // [x1, y1, x2, y2) of the slot's paste; x2 = 0 for a slot that holds nothing
    __shared__ unsigned long long accL[MS_MAXK * MYOLO_MEASURE_WORDS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y;
    const int H = frames[2 * b], W = frames[2 * b + 1];
    const int tiles_x = (W + MS_TW - 1) / MS_TW, tiles_y = (H + MS_TH - 1) / MS_TH;
    const int ntiles = tiles_x * tiles_y;                          // (h, w <= 32768: at most 2^19)
    if ((int)blockIdx.x * 4 >= ntiles) return;                     // the grid is the largest image's: uniform over the workgroup

    for (int k = tid; k < K; k += 256) {
        const int s = sel[b * K + k];
        int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        if (s >= 0 && s < R) unmold_window(det + ((long long)b * R + s) * 6, H, W, x1, y1, x2, y2);
        if (x2 <= x1 || y2 <= y1) x1 = y1 = x2 = y2 = 0;
        winL[k][0] = x1, winL[k][1] = y1, winL[k][2] = x2, winL[k][3] = y2;
    }
    for (int i = tid; i < K * MYOLO_MEASURE_WORDS; i += 256) {
        const int word = i % MYOLO_MEASURE_WORDS;
        accL[i] = (word == 9 || word == 10) ? MS_NONE : 0ull;
    }
    __syncthreads();

    const int t = blockIdx.x * 4 + wave;
    if (t < ntiles) {                                              // the same for the whole wave, as is everything that decides a branch below
        const int tx0 = (t % tiles_x) * MS_TW, ty0 = (t / tiles_x) * MS_TH;
        const int x = tx0 + lane;
        const int nrows = min(MS_TH, H - ty0);                     // the tile's rows inside the frame; bits nrows .. 31 of a word stay 0
        const unsigned rowmask = nrows == 32 ? 0xFFFFFFFFu : ((1u << nrows) - 1u);
        const bool last_row = ty0 + nrows == H;                    // the frame's bottom edge lies under bit nrows - 1
        unsigned covered = 0;
        for (int k = 0; k < K; ++k) {
            const int x1 = winL[k][0], y1 = winL[k][1], x2 = winL[k][2], y2 = winL[k][3];
            // an empty slot or window (sel may be -1: nothing below may be read), or no pixel of the window in the tile, its left column or the
            // row above it
            if (x2 <= x1 || x2 <= tx0 - 1 || x1 >= tx0 + MS_TW || y2 <= ty0 - 1 || y1 >= ty0 + MS_TH) continue;
            const long long row = (long long)b * R + sel[b * K + k];
            const float* d = det + row * 6;
            const float* m0 = masks + row * mh * mw * C;
            const int ah = allhigh[b * K + k];
            unsigned w = 0;
            const int ya = max(ty0, y1), yb = min(ty0 + MS_TH, y2);
            for (int y = ya; y < yb; ++y) w |= (unsigned)unmold_pixel(d, m0, ah, x, y, mh, mw, C, H, W) << (y - ty0);
            const unsigned above = unmold_pixel(d, m0, ah, x, ty0 - 1, mh, mw, C, H, W);
            int hv = 0;                                            // lanes 0 .. 31: the column left of the tile; lane 32: the corner above it
            if (lane <= 32) hv = unmold_pixel(d, m0, ah, tx0 - 1, lane < 32 ? ty0 + lane : ty0 - 1, mh, mw, C, H, W);
            const unsigned long long halo = __ballot(hv);
            const unsigned long long cols = __ballot(w != 0);      // the tile's columns that hold a pixel
            if (!(cols | halo | __ballot(above))) continue;
            unsigned left = __shfl_up(w, 1), labove = __shfl_up(above, 1);
            if (lane == 0) left = (unsigned)halo, labove = (unsigned)(halo >> 32) & 1u;
            const unsigned n = __popc(w), vis = __popc(w & ~covered);
            covered |= w;
            const unsigned wu = (w << 1) | above, lu = (left << 1) | labove;
            unsigned per = __popc((w ^ wu) & rowmask) + (last_row ? (w >> (nrows - 1)) & 1u : 0u);
            if (x < W) per += __popc(w ^ left) + (x == W - 1 ? n : 0u);
            const unsigned quads = __popc(w & left & wu & lu);
            unsigned s1, s2;
            ms_bit_index_sums(w, s1, s2);
            // wave sums; the small ones share a word: n, vis <= 2048, per <= 97 * 64, quads <= 2048, sum i <= 496 * 64, l * n <= 2016 * 32 < 2^16
            const unsigned lx = lane;
            const unsigned p0 = ms_wave_sum(n | (vis << 16)), p1 = ms_wave_sum(per | (quads << 16)), p2 = ms_wave_sum(s1 | ((lx * n) << 16));
            const long long S2 = ms_wave_sum(s2), LXXN = ms_wave_sum(lx * lx * n), LXS1 = ms_wave_sum(lx * s1);
            const unsigned rows = ms_wave_or(w);
            const long long N = p0 & 0xFFFFu, S1 = p2 & 0xFFFFu, LXN = p2 >> 16;
            const long long X0 = tx0, Y0 = ty0;
            unsigned long long v = 0;
            switch (lane) {
            case 0: v = N; break;
            case 1: v = p0 >> 16; break;
            case 2: v = X0 * N + LXN; break;
            case 3: v = Y0 * N + S1; break;
            case 4: v = X0 * X0 * N + 2 * X0 * LXN + LXXN; break;
            case 5: v = Y0 * Y0 * N + 2 * Y0 * S1 + S2; break;
            case 6: v = X0 * Y0 * N + X0 * S1 + Y0 * LXN + LXS1; break;
            case 7: v = p1 & 0xFFFFu; break;
            case 8: v = p1 >> 16; break;
            case 9: v = cols ? (unsigned long long)(tx0 + __ffsll((long long)cols) - 1) : MS_NONE; break;
            case 10: v = rows ? (unsigned long long)(ty0 + __ffs((int)rows) - 1) : MS_NONE; break;
            case 11: v = cols ? (unsigned long long)(tx0 + 64 - __clzll((long long)cols)) : 0ull; break;
            case 12: v = rows ? (unsigned long long)(ty0 + 32 - __clz((int)rows)) : 0ull; break;
            default: break;
            }
            if (lane < MYOLO_MEASURE_WORDS) {
                unsigned long long* a = accL + k * MYOLO_MEASURE_WORDS + lane;
                if (lane == 9 || lane == 10) atomicMin(a, v);
                else if (lane == 11 || lane == 12) atomicMax(a, v);
                else if (v) atomicAdd(a, v);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < K * MYOLO_MEASURE_WORDS; i += 256) {
        const int word = i % MYOLO_MEASURE_WORDS;
        const unsigned long long v = accL[i];
        unsigned long long* o = out + (long long)b * K * MYOLO_MEASURE_WORDS + i;
        if (word == 9 || word == 10) {
            if (v != MS_NONE) atomicMin(o, v);
        } else if (v) {
            if (word == 11 || word == 12) atomicMax(o, v);
            else atomicAdd(o, v);
        }
    }
}

// ---------------------------------------------------------------------------------------
// GPU producer of the Shapes input pipeline: rasterise the images and instance masks
// of a batch from their shape specifications (example/shapes/dataset_shapes.py:80-135: load_image / load_mask /
// draw_shape incl. the occlusion rule :112-116), drop empty instances and take tight boxes (load_image_gt + extract_bboxes,
// myolo_utils.py:247-271,346-352), and encode the YOLO targets (BatchGenerator.__getitem__, myolo_utils.py:753-844).
// spec layout per image (int32): [bg_r, bg_g, bg_b, n_shapes] then SHAPE_INTS per shape:
//   [type(1 square, 2 circle, 3 triangle), r, g, b, x, y, s, ax, ay, bx, by, cx, cy]  (triangle vertices already int-truncated)
// ---------------------------------------------------------------------------------------
#define SHAPE_INTS 13
#define SPEC_MAXS 8

__device__ __forceinline__ bool shape_covers(const int* sp, int px, int py)
{
    const int type = sp[0], x = sp[4], y = sp[5], s = sp[6];
    if (type == 1) return px >= x - s && px <= x + s && py >= y - s && py <= y + s;
    if (type == 2) return (px - x) * (px - x) + (py - y) * (py - y) <= s * s;
    const int ax = sp[7], ay = sp[8], bx = sp[9], by = sp[10], cx = sp[11], cy = sp[12];
    const int e0 = (px - ax) * (by - ay) - (py - ay) * (bx - ax);
    const int e1 = (px - bx) * (cy - by) - (py - by) * (cx - bx);
    const int e2 = (px - cx) * (ay - cy) - (py - cy) * (ax - cx);
    return (e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0);
}

__global__ void shapes_stats_init_kernel(int* stats, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { stats[i * 5 + 0] = 0; stats[i * 5 + 1] = 0x7fffffff; stats[i * 5 + 2] = -1; stats[i * 5 + 3] = 0x7fffffff; stats[i * 5 + 4] = -1; }
}

// pass 1: per (image, shape) visible-pixel count and extent.  stats[b][s] = {count, minx, maxx, miny, maxy}
__global__ __launch_bounds__(256) void shapes_stats_kernel(const int* __restrict__ spec, int spec_stride, int* __restrict__ stats,
                                                           int H, int W, int S)
{
    const int b = blockIdx.y;
    const int* sp = spec + (long long)b * spec_stride;
    const int n = sp[3];
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= H * W) return;
    const int py = pix / W, px = pix - py * W;
    bool later = false;
    for (int k = n - 1; k >= 0; --k) {          // walk from the last drawn shape: it occludes the earlier ones
        const bool in = shape_covers(sp + 4 + k * SHAPE_INTS, px, py);
        if (in && !later) {
            int* st = stats + ((long long)b * S + k) * 5;
            atomicAdd(st + 0, 1);
            atomicMin(st + 1, px); atomicMax(st + 2, px);
            atomicMin(st + 3, py); atomicMax(st + 4, py);
        }
        later = later || in;
    }
}

// pass 2 (one workgroup per image): compaction of non-empty instances, boxes, class ids, YOLO target encoding
__global__ void shapes_encode_kernel(const int* __restrict__ spec, int spec_stride, const int* __restrict__ stats, int* __restrict__ slotmap,
                                     int32_t* __restrict__ gt_ids, int32_t* __restrict__ gt_boxes, float* __restrict__ y_true,
                                     float* __restrict__ true_boxes, const double* __restrict__ anchors, int H, int W, int S, int T,
                                     int G, int A, int C)
{
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int* sp = spec + (long long)b * spec_stride;
    const int n = sp[3];
    const double cell_w = (double)W / G, cell_h = (double)H / G;
    int m = 0, tbi = 0;
    for (int k = 0; k < S; ++k) slotmap[b * S + k] = -1;
    for (int k = 0; k < n; ++k) {
        const int* st = stats + ((long long)b * S + k) * 5;
        if (st[0] <= 0 || m >= T) continue;                   // np.sum(mask) > 0 filter (myolo_utils.py:346)
        slotmap[b * S + k] = m;
        const int x1 = st[1], x2 = st[2] + 1, y1 = st[3], y2 = st[4] + 1;     // extract_bboxes: x2, y2 exclusive
        const int cls = sp[4 + k * SHAPE_INTS];
        gt_ids[b * T + m] = cls;
        int32_t* gb = gt_boxes + ((long long)b * T + m) * 4;
        gb[0] = x1; gb[1] = y1; gb[2] = x2; gb[3] = y2;
        const double cx = .5 * (x1 + x2) / cell_w, cy = .5 * (y1 + y2) / cell_h;
        const int gx = (int)floor(cx), gy = (int)floor(cy);
        if (gx < G && gy < G) {
            const double bw = (x2 - x1) / cell_w, bh = (y2 - y1) / cell_h;
            int best = -1;
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
            yt[5 + cls] = 1.0f;
            float* tb = true_boxes + ((long long)b * T + tbi) * 4;
            tb[0] = (float)cx; tb[1] = (float)cy; tb[2] = (float)bw; tb[3] = (float)bh;
            tbi = (tbi + 1) % T;
        }
        ++m;
    }
}

// pass 3: pixels -- image (uint8 colour / 255 through a host-provided table) and instance masks in compacted order
__global__ __launch_bounds__(256) void shapes_render_kernel(const int* __restrict__ spec, int spec_stride, const int* __restrict__ slotmap,
                                                            const float* __restrict__ lut, float* __restrict__ images,
                                                            uint8_t* __restrict__ masks, int H, int W, int S, int T)
{
    const int b = blockIdx.y;
    const int* sp = spec + (long long)b * spec_stride;
    const int n = sp[3];
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= H * W) return;
    const int py = pix / W, px = pix - py * W;
    int r = sp[0], g = sp[1], bl = sp[2];
    uint8_t* mp = masks + ((long long)b * H * W + pix) * T;
    for (int t = 0; t < T; ++t) mp[t] = 0;
    bool later = false;
    for (int k = n - 1; k >= 0; --k) {
        const int* s1 = sp + 4 + k * SHAPE_INTS;
        const bool in = shape_covers(s1, px, py);
        if (in && !later) {
            r = s1[1]; g = s1[2]; bl = s1[3];               // the top-most shape gives the pixel its colour
            const int slot = slotmap[b * S + k];
            if (slot >= 0) mp[slot] = 1;
        }
        later = later || in;
    }
    float* ip = images + ((long long)b * H * W + pix) * 3;
    ip[0] = lut[r & 255]; ip[1] = lut[g & 255]; ip[2] = lut[bl & 255];
}

extern "C" {

int myolo_yolo_decode(const float* y_pred, const float* anchors, float* proposals, int B, int G, int A, int C, void* stream)
{
    MYOLO_REQUIRE(y_pred && anchors && proposals && B > 0 && G > 0 && A > 0 && C > 0, "yolo_decode: bad arguments");
    const int total = B * G * G * A;
    hipLaunchKernelGGL(yolo_decode_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, y_pred, anchors,
                       proposals, total, G, A, 5 + C, 0);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_yolo_detections(const float* y_pred, const float* anchors, float* detections, int B, int G, int A, int C, void* stream)
{
    MYOLO_REQUIRE(y_pred && anchors && detections && B > 0 && G > 0 && A > 0 && C > 0, "yolo_detections: bad arguments");
    const int total = B * G * G * A;
    hipLaunchKernelGGL(yolo_decode_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, y_pred, anchors,
                       detections, total, G, A, 5 + C, 1);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_shapes_batch(const int32_t* spec, int spec_stride, const double* anchors, const float* lut, float* images, uint8_t* gt_masks,
                       int32_t* gt_boxes, int32_t* gt_class_ids, float* y_true, float* true_boxes, int B, int H, int W, int S, int T,
                       int G, int A, int C, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(spec && anchors && lut && images && gt_masks && gt_boxes && gt_class_ids && y_true && true_boxes, "shapes_batch: null pointer");
    MYOLO_REQUIRE(B > 0 && H > 0 && W > 0 && S > 0 && S <= SPEC_MAXS && T > 0 && spec_stride >= 4 + S * SHAPE_INTS, "shapes_batch: bad sizes");
    const size_t need = (size_t)B * S * 6 * sizeof(int);
    MYOLO_NEED_WS(need);
    int* stats = (int*)ws;
    int* slotmap = stats + (size_t)B * S * 5;
    hipStream_t s = (hipStream_t)stream;
    // stats init: count 0, min = INT_MAX, max = -1  (pattern fill through a tiny kernel-free trick: two memsets)
    (void)hipMemsetAsync(stats, 0, (size_t)B * S * 5 * sizeof(int), s);
    (void)hipMemsetAsync(gt_boxes, 0, (size_t)B * T * 4 * sizeof(int32_t), s);
    (void)hipMemsetAsync(gt_class_ids, 0, (size_t)B * T * sizeof(int32_t), s);
    (void)hipMemsetAsync(y_true, 0, (size_t)B * G * G * A * (5 + C) * sizeof(float), s);
    (void)hipMemsetAsync(true_boxes, 0, (size_t)B * T * 4 * sizeof(float), s);
    hipLaunchKernelGGL(shapes_stats_init_kernel, dim3((B * S + 255) / 256), dim3(256), 0, s, stats, B * S);
    dim3 grid((H * W + 255) / 256, B);
    hipLaunchKernelGGL(shapes_stats_kernel, grid, dim3(256), 0, s, spec, spec_stride, stats, H, W, S);
    hipLaunchKernelGGL(shapes_encode_kernel, dim3(B), dim3(64), 0, s, spec, spec_stride, stats, slotmap, gt_class_ids, gt_boxes, y_true,
                       true_boxes, anchors, H, W, S, T, G, A, C);
    hipLaunchKernelGGL(shapes_render_kernel, grid, dim3(256), 0, s, spec, spec_stride, slotmap, lut, images, gt_masks, H, W, S, T);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_unmold_masks(const float* masks, const float* detections, uint8_t* full_masks, int N, int mh, int mw, int C, int H,
                       int W, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(masks && detections && full_masks && N > 0 && mh > 0 && mw > 0 && C > 0 && H > 0 && W > 0, "unmold_masks: bad arguments");
    MYOLO_NEED_WS((size_t)N * sizeof(int32_t));
    int32_t* allhigh = (int32_t*)ws;
    hipLaunchKernelGGL(unmold_allhigh_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, masks, detections, allhigh, mh, mw, C,
                       (const int32_t*)nullptr, 1, N);
    const long long total = (long long)H * W * N;
    long long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(unmold_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, masks, detections, allhigh, full_masks, N,
                       mh, mw, C, H, W);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_mask_overlap_counts(const float* masks, const float* det, const int32_t* sel, const int32_t* sel_host, const uint8_t* gt_masks,
                              int32_t* inter, int32_t* area_pred, int32_t* area_gt, int32_t* win, int B, int R, int K, int T, int mh, int mw,
                              int C, int H, int W, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(masks && det && sel && sel_host && gt_masks && inter && area_pred && area_gt && win, "mask_overlap_counts: null pointer");
    MYOLO_REQUIRE(B > 0 && R > 0 && mh > 0 && mw > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) - 64,
                  "mask_overlap_counts: bad sizes");
    MYOLO_REQUIRE(K > 0 && K <= OV_MAXK && T > 0 && T <= OV_MAXT, "mask_overlap_counts: need 1 <= K <= %d and 1 <= T <= %d (got K=%d, T=%d)",
                  OV_MAXK, OV_MAXT, K, T);
    for (long long i = 0; i < (long long)B * K; ++i)
        MYOLO_REQUIRE(sel_host[i] < R, "mask_overlap_counts: sel[%lld] = %d is not a row of the %d detections", i, sel_host[i], R);
    MYOLO_REQUIRE(ws && ws_bytes >= (size_t)B * K * sizeof(int32_t), "mask_overlap_counts: workspace too small (%zu needed, %zu given)",
                  (size_t)B * K * sizeof(int32_t), ws_bytes);
    int32_t* allhigh = (int32_t*)ws;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(inter, 0, (size_t)B * K * T * sizeof(int32_t), s);
    (void)hipMemsetAsync(area_pred, 0, (size_t)B * K * sizeof(int32_t), s);
    (void)hipMemsetAsync(area_gt, 0, (size_t)B * T * sizeof(int32_t), s);
    hipLaunchKernelGGL(unmold_allhigh_kernel, dim3(B * K), dim3(256), 0, s, masks, det, allhigh, mh, mw, C, sel, K, R);
    const int ngroups = (H * W + 63) / 64;
    hipLaunchKernelGGL(mask_overlap_kernel, dim3((ngroups + OV_GROUPS - 1) / OV_GROUPS, B), dim3(256), 0, s, masks, det, sel,
                       (const int32_t*)allhigh, gt_masks, inter, area_pred, area_gt, win, R, K, T, mh, mw, C, H, W,
                       ((uintptr_t)gt_masks & 15) == 0 ? 1 : 0);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

// the B * K all-high flags, then the B * K rows of max_w column counts
size_t myolo_rle_masks_ws_bytes(int B, int K, int max_w)
{
    if (B <= 0 || K <= 0 || max_w <= 0) return 0;
    const size_t words = (size_t)B * K * ((size_t)max_w + 1);
    return (words * sizeof(int32_t) + 255) / 256 * 256;
}

int myolo_rle_masks(const float* masks, const float* det, const int32_t* sel, const int32_t* sel_host, const int32_t* frames,
                    const int32_t* frames_host, int32_t* run_off, uint32_t* bounds, int64_t cap, int B, int R, int K, int mh, int mw, int C,
                    void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(masks && det && sel && sel_host && frames && frames_host && run_off && bounds && ws, "rle_masks: null pointer");
    MYOLO_REQUIRE(B > 0 && R > 0 && mh > 0 && mw > 0 && C > 0 && cap >= 0, "rle_masks: bad sizes");
    MYOLO_REQUIRE(K > 0 && K <= OV_MAXK, "rle_masks: need 1 <= K <= %d (got K=%d)", OV_MAXK, K);
    MYOLO_REQUIRE((long long)B * K <= 65535, "rle_masks: B * K = %lld slots, more than the 65535 of one launch", (long long)B * K);
    int max_w = 0;
    long long pixels = 0;                                          // an upper bound of the boundaries of all slots: run_off is 32-bit
    for (int b = 0; b < B; ++b) {
        const int h = frames_host[2 * b], w = frames_host[2 * b + 1];
        MYOLO_REQUIRE(h >= 1 && w >= 1, "rle_masks: frame %d is %d x %d (h, w >= 1 needed)", b, h, w);
        MYOLO_REQUIRE((long long)h * w < (1ll << 31), "rle_masks: frame %d (%d x %d) has 2^31 pixels or more", b, h, w);
        pixels += (long long)h * w * K;
        max_w = w > max_w ? w : max_w;
    }
    MYOLO_REQUIRE(pixels < (1ll << 31), "rle_masks: the frames of the batch hold %lld pixels x slots, 2^31 or more", pixels);
    for (long long i = 0; i < (long long)B * K; ++i)
        MYOLO_REQUIRE(sel_host[i] < R, "rle_masks: sel[%lld] = %d is not a row of the %d detections", i, sel_host[i], R);
    const size_t need = myolo_rle_masks_ws_bytes(B, K, max_w);
    MYOLO_REQUIRE(ws_bytes >= need, "rle_masks: workspace too small (%zu needed for frames up to %d wide, %zu given)", need, max_w, ws_bytes);
    int32_t* allhigh = (int32_t*)ws;
    int32_t* cols = allhigh + (size_t)B * K;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((max_w + 3) / 4, B * K);
    hipLaunchKernelGGL(unmold_allhigh_kernel, dim3(B * K), dim3(256), 0, s, masks, det, allhigh, mh, mw, C, sel, K, R);
    hipLaunchKernelGGL(rle_columns_kernel<false>, grid, dim3(256), 0, s, masks, det, sel, (const int32_t*)allhigh, frames, cols,
                       (const int32_t*)run_off, bounds, (long long)cap, R, K, mh, mw, C, max_w);
    hipLaunchKernelGGL(rle_scan_columns_kernel, dim3(B * K), dim3(256), 0, s, cols, run_off, max_w);
    hipLaunchKernelGGL(rle_scan_slots_kernel, dim3(1), dim3(256), 0, s, run_off, B * K);
    hipLaunchKernelGGL(rle_columns_kernel<true>, grid, dim3(256), 0, s, masks, det, sel, (const int32_t*)allhigh, frames, cols,
                       (const int32_t*)run_off, bounds, (long long)cap, R, K, mh, mw, C, max_w);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

// [all-high flags B*K | rows B*K*(max_h + 1)] int32, padded to 16 bytes; then per vertex of cap: the key (8 bytes) and nine int32 words (succ, the
// double buffers of head / link / distance, the two scan rows).  Nothing grows with the frame's width, 4 * B * K bytes with a row of its height.
#define CT_WORDS_PER_VERTEX 9
static size_t contour_head_bytes(int B, int K, int max_h)
{
    const size_t words = (size_t)B * K * ((size_t)max_h + 2);
    return (words * sizeof(int32_t) + 15) / 16 * 16;
}

size_t myolo_contour_masks_ws_bytes(int B, int K, int max_h, int max_w, int64_t cap)
{
    if (B <= 0 || K <= 0 || max_h <= 0 || max_w <= 0 || cap < 0) return 0;
    return contour_head_bytes(B, K, max_h) + (size_t)cap * (sizeof(unsigned long long) + CT_WORDS_PER_VERTEX * sizeof(int32_t));
}

int myolo_contour_masks(const float* masks, const float* det, const int32_t* sel, const int32_t* sel_host, const int32_t* frames,
                        const int32_t* frames_host, int32_t* vert_off, int32_t* verts, int32_t* loop_id, int64_t cap, int B, int R, int K, int mh,
                        int mw, int C, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(masks && det && sel && sel_host && frames && frames_host && vert_off && verts && loop_id && ws, "contour_masks: null pointer");
    MYOLO_REQUIRE(B > 0 && R > 0 && mh > 0 && mw > 0 && C > 0 && cap >= 0 && cap < (1ll << 31), "contour_masks: bad sizes");
    MYOLO_REQUIRE(K > 0 && K <= OV_MAXK, "contour_masks: need 1 <= K <= %d (got K=%d)", OV_MAXK, K);
    MYOLO_REQUIRE((long long)B * K <= 65535, "contour_masks: B * K = %lld slots, more than the 65535 of one launch", (long long)B * K);
    int max_h = 0, max_w = 0;
    long long corners = 0;                                         // two vertices a corner at the most: vert_off is 32-bit
    for (int b = 0; b < B; ++b) {
        const int h = frames_host[2 * b], w = frames_host[2 * b + 1];
        MYOLO_REQUIRE(h >= 1 && w >= 1, "contour_masks: frame %d is %d x %d (h, w >= 1 needed)", b, h, w);
        MYOLO_REQUIRE((long long)h * w < (1ll << 31), "contour_masks: frame %d (%d x %d) has 2^31 pixels or more", b, h, w);
        corners += ((long long)h + 1) * ((long long)w + 1) * K;
        max_h = h > max_h ? h : max_h;
        max_w = w > max_w ? w : max_w;
    }
    MYOLO_REQUIRE(2 * corners < (1ll << 31), "contour_masks: the frames of the batch hold %lld corners x slots, 2^30 or more", corners);
    for (long long i = 0; i < (long long)B * K; ++i)
        MYOLO_REQUIRE(sel_host[i] < R, "contour_masks: sel[%lld] = %d is not a row of the %d detections", i, sel_host[i], R);
    const size_t need = myolo_contour_masks_ws_bytes(B, K, max_h, max_w, cap);
    MYOLO_REQUIRE(ws_bytes >= need, "contour_masks: workspace too small (%zu needed for frames up to %d high and %lld vertices, %zu given)", need,
                  max_h, (long long)cap, ws_bytes);
    MYOLO_REQUIRE(((uintptr_t)ws & 7) == 0, "contour_masks: the workspace must be 8-byte aligned");
    const int nslots = B * K, max_rows = max_h + 1;
    int32_t* allhigh = (int32_t*)ws;
    int32_t* rows = allhigh + nslots;
    unsigned long long* keys = (unsigned long long*)((char*)ws + contour_head_bytes(B, K, max_h));
    int32_t* w32 = (int32_t*)(keys + cap);
    int32_t* part[CT_WORDS_PER_VERTEX];
    for (int i = 0; i < CT_WORDS_PER_VERTEX; ++i) part[i] = w32 + (size_t)i * cap;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((max_rows + 3) / 4, nslots);
    hipLaunchKernelGGL(unmold_allhigh_kernel, dim3(nslots), dim3(256), 0, s, masks, det, allhigh, mh, mw, C, sel, K, R);
    hipLaunchKernelGGL(contour_rows_kernel<false>, grid, dim3(256), 0, s, masks, det, sel, (const int32_t*)allhigh, frames, rows,
                       (const int32_t*)vert_off, keys, (long long)cap, nslots, R, K, mh, mw, C, max_rows);
    hipLaunchKernelGGL(rle_scan_columns_kernel, dim3(nslots), dim3(256), 0, s, rows, vert_off, max_rows);
    hipLaunchKernelGGL(rle_scan_slots_kernel, dim3(1), dim3(256), 0, s, vert_off, nslots);
    hipLaunchKernelGGL(contour_rows_kernel<true>, grid, dim3(256), 0, s, masks, det, sel, (const int32_t*)allhigh, frames, rows,
                       (const int32_t*)vert_off, keys, (long long)cap, nslots, R, K, mh, mw, C, max_rows);
    hipLaunchKernelGGL(contour_link_kernel, dim3(CT_LINK_BLOCKS, nslots), dim3(256), 0, s, masks, det, sel, (const int32_t*)allhigh, frames,
                       (const int32_t*)vert_off, (const unsigned long long*)keys, part[0], (long long)cap, nslots, R, K, mh, mw, C);
    hipLaunchKernelGGL(contour_rank_kernel, dim3(nslots), dim3(256), 0, s, (const int32_t*)vert_off, (const unsigned long long*)keys,
                       (const int32_t*)part[0], part[1], part[2], part[3], part[4], part[5], part[6], part[7], part[8], verts, loop_id,
                       (long long)cap, nslots);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_render_instances(const uint8_t* images, uint8_t* out, size_t nbytes, const int64_t* desc, const int64_t* desc_host, const float* masks,
                           const float* det, const int32_t* sel, const int32_t* sel_host, const double* colors, double alpha, double box_alpha,
                           int flags, int B, int R, int K, int mh, int mw, int C, void* ws, size_t ws_bytes, void* stream)
{
    MYOLO_REQUIRE(images && out && desc && desc_host && masks && det && sel && sel_host && colors && ws, "render_instances: null pointer");
    MYOLO_REQUIRE(B > 0 && B <= 65535 && R > 0 && mh > 0 && mw > 0 && C > 0, "render_instances: bad sizes");
    MYOLO_REQUIRE(K > 0 && K <= OV_MAXK, "render_instances: need 1 <= K <= %d (got K=%d)", OV_MAXK, K);
    MYOLO_REQUIRE(alpha >= 0.0 && alpha <= 1.0 && box_alpha >= 0.0 && box_alpha <= 1.0 && (flags & ~(RN_BLEND | RN_OUTLINE | RN_BOX)) == 0,
                  "render_instances: alpha and box_alpha must lie in [0, 1] and flags in [0, 7] (got %g, %g, %d)", alpha, box_alpha, flags);
    MYOLO_REQUIRE(nbytes < ((size_t)1 << 31), "render_instances: a batch of %zu bytes, 2^31 or more", nbytes);
    long long tiles = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t off = desc_host[b * 3], h = desc_host[b * 3 + 1], w = desc_host[b * 3 + 2];
        MYOLO_REQUIRE(h >= 1 && w >= 1, "render_instances: frame %d is %lld x %lld (h, w >= 1 needed)", b, (long long)h, (long long)w);
        // 3 * h * w <= nbytes < 2^31 without forming a product that could overflow, then the offset
        MYOLO_REQUIRE(off >= 0 && w <= (int64_t)nbytes / 3 && h <= (int64_t)nbytes / 3 / w && off <= (int64_t)nbytes - 3 * h * w,
                      "render_instances: image %d (offset %lld, %lld x %lld x 3) does not fit the %zu bytes of the batch", b, (long long)off,
                      (long long)h, (long long)w, nbytes);
        const long long t = ((w + RN_TW - 1) / RN_TW) * ((h + RN_TH - 1) / RN_TH);
        tiles = t > tiles ? t : tiles;
    }
    for (long long i = 0; i < (long long)B * K; ++i)
        MYOLO_REQUIRE(sel_host[i] < R, "render_instances: sel[%lld] = %d is not a row of the %d detections", i, sel_host[i], R);
    const size_t need = (size_t)B * K * sizeof(int32_t);
    MYOLO_REQUIRE(ws_bytes >= need, "render_instances: workspace too small (%zu needed, %zu given)", need, ws_bytes);
    int32_t* allhigh = (int32_t*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(unmold_allhigh_kernel, dim3(B * K), dim3(256), 0, s, masks, det, allhigh, mh, mw, C, sel, K, R);
    hipLaunchKernelGGL(render_instances_kernel, dim3((unsigned)tiles, B), dim3(256), 0, s, images, out, desc, masks, det, sel,
                       (const int32_t*)allhigh, colors, alpha, box_alpha, flags, R, K, mh, mw, C);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

// the B * K all-high flags
size_t myolo_measure_masks_ws_bytes(int B, int K)
{
    if (B <= 0 || K <= 0) return 0;
    return ((size_t)B * K * sizeof(int32_t) + 255) / 256 * 256;
}

int myolo_measure_masks(const float* masks, const float* det, const int32_t* sel, const int32_t* sel_host, const int32_t* frames,
                        const int32_t* frames_host, int64_t* out, int B, int R, int K, int mh, int mw, int C, void* ws, size_t ws_bytes,
                        void* stream)
{
    MYOLO_REQUIRE(masks && det && sel && sel_host && frames && frames_host && out && ws, "measure_masks: null pointer");
    MYOLO_REQUIRE(B > 0 && B <= 65535 && R > 0 && mh > 0 && mw > 0 && C > 0, "measure_masks: bad sizes");
    MYOLO_REQUIRE(K > 0 && K <= MS_MAXK, "measure_masks: need 1 <= K <= %d (got K=%d)", MS_MAXK, K);
    long long tiles = 0;
    for (int b = 0; b < B; ++b) {
        const int h = frames_host[2 * b], w = frames_host[2 * b + 1];
        MYOLO_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "measure_masks: frame %d is %d x %d (1 <= h, w <= 32768 needed)", b, h, w);
        const long long t = (long long)((w + MS_TW - 1) / MS_TW) * ((h + MS_TH - 1) / MS_TH);
        tiles = t > tiles ? t : tiles;
    }
    for (long long i = 0; i < (long long)B * K; ++i)
        MYOLO_REQUIRE(sel_host[i] < R, "measure_masks: sel[%lld] = %d is not a row of the %d detections", i, sel_host[i], R);
    const size_t need = myolo_measure_masks_ws_bytes(B, K);
    MYOLO_REQUIRE(ws_bytes >= need, "measure_masks: workspace too small (%zu needed, %zu given)", need, ws_bytes);
    int32_t* allhigh = (int32_t*)ws;
    unsigned long long* o = (unsigned long long*)out;
    hipStream_t s = (hipStream_t)stream;
    const int nslots = B * K;
    hipLaunchKernelGGL(measure_init_kernel, dim3((nslots * MYOLO_MEASURE_WORDS + 255) / 256), dim3(256), 0, s, o, nslots);
    hipLaunchKernelGGL(unmold_allhigh_kernel, dim3(nslots), dim3(256), 0, s, masks, det, allhigh, mh, mw, C, sel, K, R);
    hipLaunchKernelGGL(measure_masks_kernel, dim3((unsigned)((tiles + 3) / 4), B), dim3(256), 0, s, masks, det, sel, (const int32_t*)allhigh,
                       frames, o, R, K, mh, mw, C);
    hipLaunchKernelGGL(measure_finish_kernel, dim3((nslots + 255) / 256), dim3(256), 0, s, o, nslots);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_mask_targets(const float* proposals, const int32_t* gt_class_ids, const int32_t* gt_boxes_px, const uint8_t* gt_masks,
                       float* rois, int32_t* target_class_ids, float* target_masks, int32_t* n_pos, int B, int R, int T, int H,
                       int W, int mh, int mw, void* stream)
{
    MYOLO_REQUIRE(proposals && gt_class_ids && gt_boxes_px && gt_masks && rois && target_class_ids && target_masks && n_pos,
                  "mask_targets: null pointer");
    MYOLO_REQUIRE(B > 0 && R > 0 && R <= MT_MAXR && T > 0 && T <= MT_MAXT && mh > 1 && mw > 1,
                  "mask_targets: need R<=%d, T<=%d, mask shape > 1", MT_MAXR, MT_MAXT);
    hipLaunchKernelGGL(mask_targets_kernel, dim3(B, B >= 128 ? 2 : 8), dim3(256), 0, (hipStream_t)stream, proposals, gt_class_ids, gt_boxes_px,
                       gt_masks, rois, target_class_ids, target_masks, n_pos, R, T, H, W, mh, mw);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

int myolo_yolo_loss(const float* y_true, const float* y_pred, const float* true_boxes, const float* anchors,
                    const float* class_weights, float object_scale, float no_object_scale, float coord_scale, float class_scale,
                    float loss_weight, float* out_terms, float* grad, int B, int G, int A, int C, int T, void* ws, size_t ws_bytes,
                    void* stream)
{
    return myolo_yolo_loss_warmup(y_true, y_pred, true_boxes, anchors, class_weights, object_scale, no_object_scale, coord_scale, class_scale,
                                  loss_weight, 0, out_terms, grad, B, G, A, C, T, ws, ws_bytes, stream);
}

int myolo_yolo_loss_warmup(const float* y_true, const float* y_pred, const float* true_boxes, const float* anchors,
                           const float* class_weights, float object_scale, float no_object_scale, float coord_scale, float class_scale,
                           float loss_weight, int warmup, float* out_terms, float* grad, int B, int G, int A, int C, int T, void* ws, size_t ws_bytes,
                           void* stream)
{
    (void)ws; (void)ws_bytes;
    MYOLO_REQUIRE(y_true && y_pred && true_boxes && anchors && class_weights && out_terms && grad, "yolo_loss: null pointer");
    MYOLO_REQUIRE(B > 0 && G > 0 && A > 0 && C > 0 && T > 0, "yolo_loss: bad sizes");
    LossArgs a{y_true, y_pred, true_boxes, anchors, class_weights, object_scale, no_object_scale, coord_scale, class_scale,
               loss_weight, out_terms, grad, B, G, A, C, T, warmup ? 1 : 0};
    hipLaunchKernelGGL(yolo_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    MYOLO_CHECK_LAUNCH();
    return MYOLO_OK;
}

}  // extern "C"
