// The training loss for gfx950: loss forward + backward (reference src/nn_skeleton.py:142-327: _add_interpretation_graph +
// _add_loss_graph) writing dL/dpreds, the same with options (IoU-family box terms, a focal class term), and
// distillation from a teacher's preds.  One kernel body per pass: the anchor addressing and its store, the
// softmax, the decode -> IoU block, the confidence term and the reduction tail each stand here once; the class and the box
// term are functions of that frame, selected at compile time (OPT) or by the options.
// Compiled with -ffp-contract=off (the loss decode must match interpret_output op for op; and moving an expression into an
// inlined function changes no rounding).
#include <math.h>

#include "train_common.h"

namespace sqdet {

struct LossArgs {
  const void* preds;       // [B, cells, K*(C+5)], float32 or (mixed-precision form) float16
  const float* anchors;    // [A,4] float32
  const float* mask;       // [B,A]
  const float* delta_in;   // [B,A,4]
  const float* box_in;     // [B,A,4] (cx,cy,w,h)
  const float* labels;     // [B,A,C]
  float* dpreds;           // [B, cells, K*(C+5)]
  f16* g16;                // mixed-precision form: (float16)(dpreds * gscale), the gradient the float16 backward starts from
  float gscale;            // (the loss scale)
  float* ious;             // [B,A]
  float* partial;          // [blocks][4]: class, conf, bbox loss partial sums (+ unused)
  int B, cells, K, C;
  int Bmean;               // divisor of the confidence loss's reduce_mean over the batch (nn_skeleton.py:304-312): B, or the
                           // GLOBAL batch when N replicas of batch B compute one graph of batch N*B (SURVEY.md 8e option b)
  float w1, h1, thr, slope, eps;
  float coef_class, coef_pos, coef_neg, coef_bbox;
  float num_obj;           // sum(mask) over the whole batch (host computed from the label tensors) ...
  const float* num_obj_dev;   // ... or, when not NULL, read from the device (sqdet_sum_f32 of the mask: no host round trip)
};
struct LossOpt { int box_loss; float gamma; };

// ------------------------------------------------------------------ the frame: one anchor of [B, A = cells * K]
// Its cell's K*(C+5) channels -- class logits at k*C + c, the confidence logit at K*C + k, the four deltas at K*(C+1) + 4k --
// and where its gradient goes.
template <typename PT>
struct Anchor {
  int an, k;
  size_t base;             // of the cell's channels, in elements
  const PT* p;
  float* dp;
  f16* gp;
  float gscale;
  __device__ __forceinline__ Anchor(long idx, const void* preds, float* dpreds, f16* g16, float gscale_, int cells, int K, int C) {
    const int A = cells * K;
    const int b = (int)(idx / A);
    an = (int)(idx - (long)b * A);
    const int cell = an / K;
    k = an - cell * K;
    base = ((size_t)b * cells + cell) * (K * (C + 5));
    p = reinterpret_cast<const PT*>(preds) + base;
    dp = dpreds + base;
    gp = g16 ? g16 + base : nullptr;
    gscale = gscale_;
  }
  // float32 dpreds, and -- float16 preds -- its loss-scaled float16 copy (convert_scale_kernel's expression) in the same pass
  __device__ __forceinline__ void put(int off, float v) const {
    dp[off] = v;
    if (sizeof(PT) == 2) gp[off] = scaled_to<f16>(v, gscale);
  }
  __device__ __forceinline__ void add(int off, float g) const { put(off, dp[off] + g); }
};

// Three per-thread sums -> a 256-wide LDS tree -> partial[block * 4 + j]; loss_finish_kernel adds the workgroups'.
__device__ __forceinline__ void block_partials(float s0, float s1, float s2, float* __restrict__ partial) {
  __shared__ float red[3][256];
  red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] += red[1][threadIdx.x + off];
      red[2][threadIdx.x] += red[2][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) partial[blockIdx.x * 4 + threadIdx.x] = threadIdx.x < 3 ? red[threadIdx.x][0] : 0.f;
}

// losses3[j] = sum over the loss kernel's workgroups of partial[b][j]: wave j of one workgroup, lane l takes b = l, l + 64, ..
// in ascending order, then a fixed xor tree -- deterministic.  (One thread per output walking up to 512 dependent loads took
// 40 us, and a device-to-device copy of the three floats followed it.)
__global__ __launch_bounds__(256) void loss_finish_kernel(const float* __restrict__ partial, float* __restrict__ losses3, int blocks) {
  const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float s = 0.f;
  for (int b = lane; b < blocks; b += 64) s += partial[b * 4 + j];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0 && j < 3) losses3[j] = s;
}

// (at most 512 workgroups: what loss_finish_kernel's workspace holds)
static int launch_blocks(long anchors) { const long b = (anchors + 255) / 256; return (int)(b > 512 ? 512 : b); }

// ------------------------------------------------------------------ class term
// Class probabilities (softmax) and their loss (nn_skeleton.py:150-160, 292-299):
//   sum_c lab * (-log(pc+eps)) + (1-lab) * (-log(1-pc+eps)),  times m * coef_class / num_objects.
// focal_gamma g > 0 (OURS):  lab * (1-pc)^g * (-log(pc+eps)) + (1-lab) * pc^g * (-log(1-pc+eps)), its derivative in pc
// exact, the modulating factor's included: d(b^g)/db = g * b^g / b, taken as 0 where b == 0 (there the other factor, the
// log, is 0 as well).  g == 0 is the reference expression itself, no powf.
struct Softmax { float mx, inv; };

template <typename PT>
__device__ __forceinline__ Softmax softmax_of(const PT* lg, int C) {
  float mx = (float)lg[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, (float)lg[c]);
  float sum = expf((float)lg[0] - mx);
  for (int c = 1; c < C; ++c) sum = sum + expf((float)lg[c] - mx);
  return {mx, 1.0f / sum};
}

// one class's term f(pc) and df/dpc
__device__ __forceinline__ void focal_term(float pc, float lab, float eps, float g, float& f, float& df) {
  const float lp = -logf(pc + eps), lq = -logf(1.0f - pc + eps);
  if (g == 0.f) {
    f = lab * lp + (1.0f - lab) * lq;
    df = -lab / (pc + eps) + (1.0f - lab) / (1.0f - pc + eps);
    return;
  }
  const float q = fmaxf(1.0f - pc, 0.0f);
  const float qg = powf(q, g), pg = powf(pc, g);
  const float dqg = q > 0.f ? g * qg / q : 0.f, dpg = pc > 0.f ? g * pg / pc : 0.f;
  f = lab * (qg * lp) + (1.0f - lab) * (pg * lq);
  df = lab * (-dqg * lp - qg / (pc + eps)) + (1.0f - lab) * (dpg * lq + pg / (1.0f - pc + eps));
}

// adds the anchor's terms to l_class (not yet divided by num_objects) one class at a time, and writes the C logit gradients
template <typename PT>
__device__ __forceinline__ void class_term(const LossArgs& a, float gamma, const Anchor<PT>& f, long idx, float m, float nobj,
                                           float& l_class) {
  const PT* lg = f.p + f.k * a.C;
  const Softmax s = softmax_of(lg, a.C);
  if (gamma != 0.f && m == 0.f) {
    // an unlabelled anchor's term and gradient are m * (finite) = 0: no powf for it (nearly every anchor: the focal launch
    // took 46 us against 25 us before this branch, batch 20)
    for (int c = 0; c < a.C; ++c) f.put(f.k * a.C + c, 0.f);
    return;
  }
  float gdotp = 0.f;
  for (int c = 0; c < a.C; ++c) {
    const float pc = expf((float)lg[c] - s.mx) * s.inv;
    float t, df;
    focal_term(pc, a.labels[idx * a.C + c], a.eps, gamma, t, df);
    l_class += t * m * a.coef_class;
    const float gc = m * a.coef_class / nobj * df;
    gdotp += gc * pc;
  }
  for (int c = 0; c < a.C; ++c) {
    const float pc = expf((float)lg[c] - s.mx) * s.inv;
    float t, df;
    focal_term(pc, a.labels[idx * a.C + c], a.eps, gamma, t, df);
    const float gc = m * a.coef_class / nobj * df;
    f.put(f.k * a.C + c, pc * (gc - gdotp));
  }
}

// ------------------------------------------------------------------ decode -> IoU with the ground-truth box
// The decode as interpret_output (nn_skeleton.py:240-269), bbox_transform of the clipped box and of the ground truth
// (utils/util.py:167-179), _tensor_iou (:241-262).
struct Decoded {
  float dl[4];                  // the four deltas
  f32x4 anc;
  float ew, eh;                 // safe_exp of the width / height delta
  float rx0, ry0, rx1, ry1;     // the raw (unclipped) edges
  float ax0, ay0, ax1, ay1;     // the prediction: the clipped box with its '+1' sides
  float bx0, by0, bx1, by1;     // the ground truth
  float iwr, ihr, iw, ih;       // the intersection's sides, before and after max(0, .)
  float inter, uni, iou1;       // iou1 = inter / (uni + eps): `ious` holds iou1 * m
};

template <typename PT>
__device__ __forceinline__ Decoded decode_iou(const LossArgs& a, const Anchor<PT>& f, long idx) {
  Decoded d;
  const PT* dlp = f.p + a.K * (a.C + 1) + 4 * f.k;
  for (int j = 0; j < 4; ++j) d.dl[j] = (float)dlp[j];
  d.anc = *reinterpret_cast<const f32x4*>(a.anchors + (size_t)f.an * 4);
  const float cx = d.anc[0] + d.dl[0] * d.anc[2];
  const float cy = d.anc[1] + d.dl[1] * d.anc[3];
  d.ew = d.dl[2] > a.thr ? a.slope * ((d.dl[2] - a.thr) + 1.0f) : expf(d.dl[2]);
  d.eh = d.dl[3] > a.thr ? a.slope * ((d.dl[3] - a.thr) + 1.0f) : expf(d.dl[3]);
  const float bw = d.anc[2] * d.ew, bh = d.anc[3] * d.eh;
  d.rx0 = cx - bw / 2.0f; d.ry0 = cy - bh / 2.0f; d.rx1 = cx + bw / 2.0f; d.ry1 = cy + bh / 2.0f;
  const float xmin = fminf(fmaxf(0.0f, d.rx0), a.w1), ymin = fminf(fmaxf(0.0f, d.ry0), a.h1);
  const float xmax = fmaxf(fminf(a.w1, d.rx1), 0.0f), ymax = fmaxf(fminf(a.h1, d.ry1), 0.0f);
  const float w2 = xmax - xmin + 1.0f, h2 = ymax - ymin + 1.0f;
  const float dcx = xmin + 0.5f * w2, dcy = ymin + 0.5f * h2;
  d.ax0 = dcx - w2 / 2.0f; d.ay0 = dcy - h2 / 2.0f; d.ax1 = dcx + w2 / 2.0f; d.ay1 = dcy + h2 / 2.0f;
  const f32x4 gb = *reinterpret_cast<const f32x4*>(a.box_in + idx * 4);
  d.bx0 = gb[0] - gb[2] / 2.0f; d.by0 = gb[1] - gb[3] / 2.0f; d.bx1 = gb[0] + gb[2] / 2.0f; d.by1 = gb[1] + gb[3] / 2.0f;
  d.iwr = fminf(d.ax1, d.bx1) - fmaxf(d.ax0, d.bx0); d.ihr = fminf(d.ay1, d.by1) - fmaxf(d.ay0, d.by0);
  d.iw = fmaxf(0.0f, d.iwr);
  d.ih = fmaxf(0.0f, d.ihr);
  d.inter = d.iw * d.ih;
  d.uni = (d.ax1 - d.ax0) * (d.ay1 - d.ay0) + (d.bx1 - d.bx0) * (d.by1 - d.by0) - d.inter;
  d.iou1 = d.inter / (d.uni + a.eps);
  return d;
}

// ------------------------------------------------------------------ confidence term
// (:304-312): mean over the batch of sum_a (iou - conf)^2 * w_a.  confidence(): the anchor's conf, read by the kernel AHEAD of
// the decode -- the stores that follow go through pointers the compiler must take to alias preds, so a load placed after them
// waits for them (the loss launch was 0.3 us, the focal one 1 us slower with the logit read here).  conf_term returns the anchor's
// term and writes its logit's gradient.
template <typename PT>
__device__ __forceinline__ float confidence(const LossArgs& a, const Anchor<PT>& f) {
  const float zc = (float)f.p[a.K * a.C + f.k];
  return 1.0f / (1.0f + expf(-zc));
}

template <typename PT>
__device__ __forceinline__ float conf_term(const LossArgs& a, const Anchor<PT>& f, float m, float nobj, float iou, float conf) {
  const float wgt = m * a.coef_pos / nobj + (1.0f - m) * a.coef_neg / ((float)(a.cells * a.K) - nobj);
  const float dc = iou - conf;
  f.put(a.K * a.C + f.k, 2.0f * (conf - iou) * wgt / (float)a.Bmean * conf * (1.0f - conf));
  return dc * dc * wgt / (float)a.Bmean;
}

// ------------------------------------------------------------------ box term
// delta_l2 (:317-323): coef_bbox * sum_a sum_d (m * (delta - delta_in))^2 / num_objects.
//
// box_loss 1..4 (OURS): coef_bbox * sum_a m * (1 - X) / num_objects on the corners the decode already has -- the
// prediction (ax0, ay0, ax1, ay1) = the clipped decoded box with its '+1' sides, the ground truth (bx0 .. by1) -- so that the
// term's IoU is the float32 value stored in `ious`.  With pw, ph / gw, gh the sides, Cw, Ch the sides of the enclosing box,
// rho2 the squared distance of the centres:
//   iou   X = IoU = inter / (uni + eps)
//   giou  X = IoU - (Cw*Ch - uni) / (Cw*Ch + eps)
//   diou  X = IoU - rho2 / (Cw^2 + Ch^2 + eps)
//   ciou  X = IoU - rho2 / (Cw^2 + Ch^2 + eps) - alpha * v,  v = 4/pi^2 * (atan(gw/gh) - atan(pw/ph))^2,
//         alpha = v / (1 - IoU + v + eps), a constant in the backward pass; dv/dpw = -8/pi^2 * (..) * ph / (pw^2 + ph^2) (the true one).
// An anchor with m == 0 takes no part in it (its ground truth is all zeros) and gets zero delta gradients.
//
// Backward: dX / d(corner) by the quotient rule on the expressions above, then the chain through  ax0 = xmin, ax1 = xmax + 1,
// xmin / xmax = clip(cx -+ bw/2, 0, w1), bw = anc_w * safe_exp(d2) (derivative exp(d2), or `slope` on the linear branch d2 > thr),
// cx = anc_x + d0 * anc_w:   dL/dd0 = anc_w * (g_x0 + g_x1),  dL/dd2 = anc_w * safe_exp'(d2) / 2 * (g_x1 - g_x0); y alike.
//
// TIE RULE (one rule for every min, max and clip): a coordinate of the prediction receives gradient through a min / max / clip
// only where it is STRICTLY the selected argument; at equality the other argument -- the ground truth's coordinate, the 0 of
// the intersection's max(0, .), the image border -- takes it, and nothing flows.  So
//   min(ax1, bx1) passes to ax1 iff ax1 < bx1, max(ax0, bx0) to ax0 iff ax0 > bx0 (intersection; and only if its side is > 0),
//   max(ax1, bx1) passes to ax1 iff ax1 > bx1, min(ax0, bx0) to ax0 iff ax0 < bx0 (enclosing box),
//   an edge passes the clip iff 0 < cx -+ bw/2 < w1: an edge exactly on the border counts as clipped.
// tests/loss_options_reference.py restates the same rule in NumPy.
//
// Adds the anchor's term to l_bbox and writes the four delta gradients.  OPT: l_bbox is divided by num_objects by the caller.
template <bool OPT, typename PT>
__device__ __forceinline__ void box_term(const LossArgs& a, int box_loss, const Anchor<PT>& f, const Decoded& d, long idx, float m,
                                         float nobj, float& l_bbox) {
  const int doff = a.K * (a.C + 1) + 4 * f.k;
  if (box_loss == 0) {
    for (int j = 0; j < 4; ++j) {
      const float df = m * (d.dl[j] - a.delta_in[idx * 4 + j]);
      // THE ONE DIFFERENCE of the two paths' delta_l2: the reference path divides every term by num_objects before it is summed,
      // as the reference does; the path with options sums first and divides once, as both do for the class term
      if (OPT) l_bbox += a.coef_bbox * (df * df);
      else l_bbox += a.coef_bbox * df * df / nobj;
      f.put(doff + j, 2.0f * a.coef_bbox * m * df / nobj);
    }
    return;
  }
  if (m == 0.f) {
    for (int j = 0; j < 4; ++j) f.put(doff + j, 0.f);
    return;
  }
  // corner order x0, y0, x1, y1; every flag is the tie rule of the header comment
  const float pw = d.ax1 - d.ax0, ph = d.ay1 - d.ay0, gw = d.bx1 - d.bx0, gh = d.by1 - d.by0;
  const float fx = d.iwr > 0.f ? 1.f : 0.f, fy = d.ihr > 0.f ? 1.f : 0.f;
  const float di[4] = {d.ax0 > d.bx0 ? -fx * d.ih : 0.f, d.ay0 > d.by0 ? -fy * d.iw : 0.f, d.ax1 < d.bx1 ? fx * d.ih : 0.f,
                       d.ay1 < d.by1 ? fy * d.iw : 0.f};
  const float da[4] = {-ph, -pw, ph, pw};
  const float ue = d.uni + a.eps;
  float X = d.iou1, du[4], dX[4];
  for (int j = 0; j < 4; ++j) {
    du[j] = da[j] - di[j];
    dX[j] = (di[j] - d.iou1 * du[j]) / ue;
  }
  if (box_loss >= 2) {
    const float Cw = fmaxf(d.ax1, d.bx1) - fminf(d.ax0, d.bx0), Ch = fmaxf(d.ay1, d.by1) - fminf(d.ay0, d.by0);
    const float sx0 = d.ax0 < d.bx0 ? -1.f : 0.f, sy0 = d.ay0 < d.by0 ? -1.f : 0.f, sx1 = d.ax1 > d.bx1 ? 1.f : 0.f,
                sy1 = d.ay1 > d.by1 ? 1.f : 0.f;
    if (box_loss == 2) {
      const float Ca = Cw * Ch, ce = Ca + a.eps;
      const float T = (Ca - d.uni) / ce;
      const float dC[4] = {sx0 * Ch, sy0 * Cw, sx1 * Ch, sy1 * Cw};
      X = X - T;
      for (int j = 0; j < 4; ++j) dX[j] = dX[j] - ((dC[j] - du[j]) - T * dC[j]) / ce;
    } else {
      const float c2e = (Cw * Cw + Ch * Ch) + a.eps;
      const float ex = (d.ax0 + d.ax1) * 0.5f - (d.bx0 + d.bx1) * 0.5f, ey = (d.ay0 + d.ay1) * 0.5f - (d.by0 + d.by1) * 0.5f;
      const float D = (ex * ex + ey * ey) / c2e;
      const float dr[4] = {ex, ey, ex, ey};
      const float dc2[4] = {2.0f * Cw * sx0, 2.0f * Ch * sy0, 2.0f * Cw * sx1, 2.0f * Ch * sy1};
      X = X - D;
      for (int j = 0; j < 4; ++j) dX[j] = dX[j] - (dr[j] - D * dc2[j]) / c2e;
      if (box_loss == 4) {
        const float k4 = 0.40528473456935109f;       // 4 / pi^2
        const float dat = atanf(gw / gh) - atanf(pw / ph);
        const float v = k4 * dat * dat;
        const float alpha = v / (((1.0f - d.iou1) + v) + a.eps);
        const float s2 = pw * pw + ph * ph;
        const float vw = -2.0f * k4 * dat * ph / s2, vh = 2.0f * k4 * dat * pw / s2;      // dv/dpw, dv/dph
        const float dv[4] = {-vw, -vh, vw, vh};
        X = X - alpha * v;
        for (int j = 0; j < 4; ++j) dX[j] = dX[j] - alpha * dv[j];
      }
    }
  }
  const float sc = a.coef_bbox * m / nobj;
  l_bbox += a.coef_bbox * m * (1.0f - X);
  const float gx0 = d.rx0 > 0.f && d.rx0 < a.w1 ? -sc * dX[0] : 0.f, gy0 = d.ry0 > 0.f && d.ry0 < a.h1 ? -sc * dX[1] : 0.f;
  const float gx1 = d.rx1 > 0.f && d.rx1 < a.w1 ? -sc * dX[2] : 0.f, gy1 = d.ry1 > 0.f && d.ry1 < a.h1 ? -sc * dX[3] : 0.f;
  const float dew = d.dl[2] > a.thr ? a.slope : d.ew, deh = d.dl[3] > a.thr ? a.slope : d.eh;
  f.put(doff + 0, d.anc[2] * (gx0 + gx1));
  f.put(doff + 1, d.anc[3] * (gy0 + gy1));
  f.put(doff + 2, 0.5f * d.anc[2] * dew * (gx1 - gx0));
  f.put(doff + 3, 0.5f * d.anc[3] * deh * (gy1 - gy0));
}

// ------------------------------------------------------------------ the loss kernel
// A thread per anchor in a grid-stride loop, per-thread sums in index order.  OPT == false is the reference's loss (the class
// and box term fixed at compile time: sqdet_loss_fwd_bwd / _dev / _mixed); OPT == true takes both from `o`
// (sqdet_loss_fwd_bwd_opt with anything but the defaults).
template <typename PT, bool OPT>
__global__ __launch_bounds__(256) void loss_kernel(LossArgs a, LossOpt o) {
  const float nobj = a.num_obj_dev ? a.num_obj_dev[0] : a.num_obj;
  const long total = (long)a.B * a.cells * a.K;
  float l_class = 0.f, l_conf = 0.f, l_bbox = 0.f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const Anchor<PT> f(idx, a.preds, a.dpreds, a.g16, a.gscale, a.cells, a.K, a.C);
    const float m = a.mask[idx];
    class_term(a, OPT ? o.gamma : 0.f, f, idx, m, nobj, l_class);
    const float conf = confidence(a, f);
    const Decoded d = decode_iou(a, f, idx);
    const float iou = d.iou1 * m;
    a.ious[idx] = iou;
    l_conf += conf_term(a, f, m, nobj, iou, conf);
    box_term<OPT>(a, OPT ? o.box_loss : 0, f, d, idx, m, nobj, l_bbox);
  }
  block_partials(l_class / nobj, l_conf, OPT ? l_bbox / nobj : l_bbox, a.partial);
}

// ------------------------------------------------------------------ distillation (OURS: not in the reference)
// A teacher's preds as a second target (sqdet_distill_fwd_bwd; the definition stands in include/sqdet.h and, sequentially, in
// tests/distill_reference.py).  The loss kernel's shape and frame.  Runs after the loss launch: every channel's own gradient g is
// formed completely, then dpreds = dpreds + g and -- float16 student -- the loss-scaled float16 copy of that sum (Anchor::add).
// The softmaxes are re-evaluated per class instead of kept in a per-thread array (C is a run-time value: an array would live in
// scratch).  Every division by the batch is the last operation of its expression and the sums are divided once per thread, so
// that global_batch = 2 * batch halves every output exactly.
struct DistillArgs {
  const void* preds;       // student [B, cells, K*(C+5)], float32 or float16
  const void* teacher;     // teacher, the same shape, float32 or float16
  float* dpreds;           // [B, cells, K*(C+5)], read and written
  f16* g16;                // float16 student: (float16)(dpreds * gscale)
  float gscale;
  float* partial;          // [blocks][4]: class, conf, box partial sums (+ unused)
  int B, cells, K, C;
  float Bg, BgA;           // (float)global batch, and times the anchors per image
  float T, c_cls, c_conf, c_box, floor;
};

__device__ __forceinline__ float softplusf(float z) { return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z))); }

template <typename PT, typename TT>
__global__ __launch_bounds__(256) void distill_kernel(DistillArgs a) {
  const long total = (long)a.B * a.cells * a.K;
  float l_cls = 0.f, l_conf = 0.f, l_box = 0.f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const Anchor<PT> f(idx, a.preds, a.dpreds, a.g16, a.gscale, a.cells, a.K, a.C);
    const int k = f.k;
    const PT* s = f.p;
    const TT* t = reinterpret_cast<const TT*>(a.teacher) + f.base;
    // teacher confidence -> the anchor's weight; the confidence term
    const float us = (float)s[a.K * a.C + k], ut = (float)t[a.K * a.C + k];
    const float cs = 1.0f / (1.0f + expf(-us)), ct = 1.0f / (1.0f + expf(-ut));
    const float w = ct >= a.floor ? ct : 0.0f;
    l_conf += ct * (ut - us) + softplusf(us) - softplusf(ut);
    f.add(a.K * a.C + k, a.c_conf * (cs - ct) / a.BgA);
    // class term: KL(q || p) of the tempered softmaxes, through max-subtracted log-softmax
    const PT* zs = s + k * a.C;
    const TT* zt = t + k * a.C;
    float ms = (float)zs[0] / a.T, mt = (float)zt[0] / a.T;
    for (int c = 1; c < a.C; ++c) { ms = fmaxf(ms, (float)zs[c] / a.T); mt = fmaxf(mt, (float)zt[c] / a.T); }
    float ss = expf((float)zs[0] / a.T - ms), st = expf((float)zt[0] / a.T - mt);
    for (int c = 1; c < a.C; ++c) { ss = ss + expf((float)zs[c] / a.T - ms); st = st + expf((float)zt[c] / a.T - mt); }
    const float ls = logf(ss), lt = logf(st);
    float kl = 0.f;
    for (int c = 0; c < a.C; ++c) {
      const float lp = ((float)zs[c] / a.T - ms) - ls, lq = ((float)zt[c] / a.T - mt) - lt;
      const float p = expf(lp), q = expf(lq);
      kl += q * (lq - lp);
      f.add(k * a.C + c, a.c_cls * a.T * w * (p - q) / a.Bg);
    }
    l_cls += w * kl;
    // box term: squared error on the four deltas
    const PT* ds = s + a.K * (a.C + 1) + 4 * k;
    const TT* dt = t + a.K * (a.C + 1) + 4 * k;
    float sq = 0.f;
    for (int d = 0; d < 4; ++d) {
      const float df = (float)ds[d] - (float)dt[d];
      sq += df * df;
      f.add(a.K * (a.C + 1) + 4 * k + d, 2.0f * a.c_box * w * df / a.Bg);
    }
    l_box += w * sq;
  }
  block_partials(a.c_cls * a.T * a.T * l_cls / a.Bg, a.c_conf * l_conf / a.BgA, a.c_box * l_box / a.Bg, a.partial);
}

}  // namespace sqdet

using namespace sqdet;

// ------------------------------------------------------------------ host side
// What a loss entry point was called with, in the parameter order of sqdet_loss_fwd_bwd_opt (include/sqdet.h): the four entries
// fill one and hand it to loss_fwd_bwd_impl.  preds_f16: float16 preds, with g16 and the loss scale.
struct LossCall {
  const void* preds; bool preds_f16; const float *anchors, *input_mask, *box_delta_input, *box_input, *labels;
  float* dpreds; void* g16; float loss_scale; float *ious, *losses3, *workspace;
  int batch, gh, gw, apg, classes;
  float img_w, img_h, exp_thresh, epsilon, coef_class, coef_conf_pos, coef_conf_neg, coef_bbox, num_objects;
  const float* num_objects_dev; int global_batch; sqdet_stream_t stream;
};

// opt NULL: the reference's loss
static int loss_fwd_bwd_impl(const LossCall& c, const LossOpt* opt) {
  SQDET_REQUIRE(c.preds && c.anchors && c.input_mask && c.box_delta_input && c.box_input && c.labels && c.dpreds && c.ious &&
                    c.losses3 && c.workspace, "loss_fwd_bwd: null pointer");
  const float num_objects = c.num_objects_dev ? 1.0f : c.num_objects;      // (read from the device: the host's value is not looked at)
  SQDET_REQUIRE(c.batch > 0 && c.gh > 0 && c.gw > 0 && c.apg > 0 && c.classes > 0 && num_objects > 0.f, "loss_fwd_bwd: bad arguments");
  SQDET_REQUIRE(c.global_batch <= 0 || c.global_batch >= c.batch, "loss_fwd_bwd: global_batch smaller than batch");
  LossArgs a;
  a.preds = c.preds; a.anchors = c.anchors; a.mask = c.input_mask; a.delta_in = c.box_delta_input; a.box_in = c.box_input;
  a.labels = c.labels; a.dpreds = c.dpreds; a.ious = c.ious; a.partial = c.workspace;
  a.g16 = c.preds_f16 ? static_cast<f16*>(c.g16) : nullptr; a.gscale = c.preds_f16 ? c.loss_scale : 1.f;
  a.B = c.batch; a.Bmean = c.global_batch > 0 ? c.global_batch : c.batch; a.cells = c.gh * c.gw; a.K = c.apg; a.C = c.classes;
  a.w1 = c.img_w - 1.0f; a.h1 = c.img_h - 1.0f; a.thr = c.exp_thresh; a.slope = (float)exp((double)c.exp_thresh); a.eps = c.epsilon;
  a.coef_class = c.coef_class; a.coef_pos = c.coef_conf_pos; a.coef_neg = c.coef_conf_neg; a.coef_bbox = c.coef_bbox;
  a.num_obj = num_objects;
  a.num_obj_dev = c.num_objects_dev;
  const int blocks = launch_blocks((long)c.batch * c.gh * c.gw * c.apg);
  const LossOpt o = opt ? *opt : LossOpt{0, 0.f};
  hipStream_t st = as_stream(c.stream);
  if (opt && c.preds_f16) hipLaunchKernelGGL((loss_kernel<f16, true>), dim3(blocks), dim3(256), 0, st, a, o);
  else if (opt) hipLaunchKernelGGL((loss_kernel<float, true>), dim3(blocks), dim3(256), 0, st, a, o);
  else if (c.preds_f16) hipLaunchKernelGGL((loss_kernel<f16, false>), dim3(blocks), dim3(256), 0, st, a, o);
  else hipLaunchKernelGGL((loss_kernel<float, false>), dim3(blocks), dim3(256), 0, st, a, o);
  SQDET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, c.workspace, c.losses3, blocks);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_loss_fwd_bwd_mixed(const void* preds_f16, const float* anchors, const float* input_mask,
                                        const float* box_delta_input, const float* box_input, const float* labels,
                                        float* dpreds, void* dpreds_scaled_f16, float loss_scale, float* ious, float* losses3,
                                        float* workspace, int batch, int gh, int gw, int apg, int classes, float img_w,
                                        float img_h, float exp_thresh, float epsilon, float coef_class, float coef_conf_pos,
                                        float coef_conf_neg, float coef_bbox, float num_objects, const float* num_objects_dev,
                                        int global_batch, sqdet_stream_t stream) {
  SQDET_REQUIRE(dpreds_scaled_f16 && loss_scale > 0.f, "loss_fwd_bwd_mixed: bad arguments");
  const LossCall c = {preds_f16, true, anchors, input_mask, box_delta_input, box_input, labels, dpreds, dpreds_scaled_f16, loss_scale,
                      ious, losses3, workspace, batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class,
                      coef_conf_pos, coef_conf_neg, coef_bbox, num_objects, num_objects_dev, global_batch, stream};
  return loss_fwd_bwd_impl(c, nullptr);
}

extern "C" int sqdet_loss_fwd_bwd_dev(const float* preds, const float* anchors, const float* input_mask,
                                      const float* box_delta_input, const float* box_input, const float* labels,
                                      float* dpreds, float* ious, float* losses3, float* workspace, int batch, int gh, int gw,
                                      int apg, int classes, float img_w, float img_h, float exp_thresh, float epsilon,
                                      float coef_class, float coef_conf_pos, float coef_conf_neg, float coef_bbox,
                                      const float* num_objects_dev, int global_batch, sqdet_stream_t stream) {
  SQDET_REQUIRE(num_objects_dev, "loss_fwd_bwd_dev: null num_objects");
  const LossCall c = {preds, false, anchors, input_mask, box_delta_input, box_input, labels, dpreds, nullptr, 1.f,
                      ious, losses3, workspace, batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class,
                      coef_conf_pos, coef_conf_neg, coef_bbox, 1.0f, num_objects_dev, global_batch, stream};
  return loss_fwd_bwd_impl(c, nullptr);
}

extern "C" int sqdet_loss_fwd_bwd(const float* preds, const float* anchors, const float* input_mask,
                                  const float* box_delta_input, const float* box_input, const float* labels,
                                  float* dpreds, float* ious, float* losses3, float* workspace, int batch, int gh, int gw,
                                  int apg, int classes, float img_w, float img_h, float exp_thresh, float epsilon,
                                  float coef_class, float coef_conf_pos, float coef_conf_neg, float coef_bbox,
                                  float num_objects, int global_batch, sqdet_stream_t stream) {
  const LossCall c = {preds, false, anchors, input_mask, box_delta_input, box_input, labels, dpreds, nullptr, 1.f,
                      ious, losses3, workspace, batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class,
                      coef_conf_pos, coef_conf_neg, coef_bbox, num_objects, nullptr, global_batch, stream};
  return loss_fwd_bwd_impl(c, nullptr);
}

// The loss with options: with the defaults it launches what the three entry points above launch.
extern "C" int sqdet_loss_fwd_bwd_opt(const void* preds, int preds_dtype, const float* anchors, const float* input_mask,
                                      const float* box_delta_input, const float* box_input, const float* labels,
                                      float* dpreds, void* dpreds_scaled_f16, float loss_scale, float* ious, float* losses3,
                                      float* workspace, int batch, int gh, int gw, int apg, int classes, float img_w,
                                      float img_h, float exp_thresh, float epsilon, float coef_class, float coef_conf_pos,
                                      float coef_conf_neg, float coef_bbox, float num_objects, const float* num_objects_dev,
                                      int global_batch, const sqdet_loss_options_t* opt, sqdet_stream_t stream) {
  SQDET_REQUIRE(opt, "loss_fwd_bwd_opt: null options");
  SQDET_REQUIRE(opt->box_loss >= SQDET_BOX_LOSS_DELTA_L2 && opt->box_loss <= SQDET_BOX_LOSS_CIOU, "loss_fwd_bwd_opt: box_loss %d is not one of 0..4", opt->box_loss);
  SQDET_REQUIRE(opt->focal_gamma >= 0.f && opt->focal_gamma < INFINITY, "loss_fwd_bwd_opt: focal_gamma must be finite and >= 0");
  SQDET_REQUIRE(preds_dtype == SQDET_F32 || preds_dtype == SQDET_F16, "loss_fwd_bwd_opt: bad dtype");
  const bool mixed = preds_dtype == SQDET_F16;
  SQDET_REQUIRE(!mixed || (dpreds_scaled_f16 && loss_scale > 0.f), "loss_fwd_bwd_opt: float16 preds need dpreds_scaled_f16 and a loss scale");
  const LossCall c = {preds, mixed, anchors, input_mask, box_delta_input, box_input, labels, dpreds, dpreds_scaled_f16, loss_scale,
                      ious, losses3, workspace, batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class,
                      coef_conf_pos, coef_conf_neg, coef_bbox, num_objects, num_objects_dev, global_batch, stream};
  const LossOpt o = {opt->box_loss, opt->focal_gamma};
  const bool defaults = opt->box_loss == SQDET_BOX_LOSS_DELTA_L2 && opt->focal_gamma == 0.f;
  return loss_fwd_bwd_impl(c, defaults ? nullptr : &o);
}

extern "C" size_t sqdet_loss_workspace_bytes(void) { return (4 * 512 + 4) * sizeof(float); }

// Distillation: distill_kernel onto the dpreds the loss launch wrote, then loss_finish_kernel into distill3.
extern "C" size_t sqdet_distill_workspace_bytes(void) { return (4 * 512 + 4) * sizeof(float); }

extern "C" int sqdet_distill_fwd_bwd(const void* preds, int preds_dtype, const void* teacher_preds, int teacher_dtype,
                                     float* dpreds_inout, void* dpreds_scaled_f16, float loss_scale, float* distill3,
                                     float* workspace, int batch, int gh, int gw, int apg, int classes, int global_batch,
                                     const sqdet_distill_options_t* opt, sqdet_stream_t stream) {
  SQDET_REQUIRE(preds && teacher_preds && dpreds_inout && distill3 && workspace && opt, "distill_fwd_bwd: null pointer");
  SQDET_REQUIRE(batch > 0 && gh > 0 && gw > 0 && apg > 0 && classes > 0, "distill_fwd_bwd: bad arguments");
  SQDET_REQUIRE(global_batch <= 0 || global_batch >= batch, "distill_fwd_bwd: global_batch smaller than batch");
  SQDET_REQUIRE(opt->temperature > 0.f && opt->temperature < INFINITY, "distill_fwd_bwd: temperature must be finite and > 0");
  const float coefs[3] = {opt->class_coef, opt->conf_coef, opt->bbox_coef};
  for (int i = 0; i < 3; ++i)
    SQDET_REQUIRE(coefs[i] >= 0.f && coefs[i] < INFINITY, "distill_fwd_bwd: coefficients must be finite and >= 0");
  SQDET_REQUIRE(coefs[0] > 0.f || coefs[1] > 0.f || coefs[2] > 0.f, "distill_fwd_bwd: all three coefficients are zero");
  SQDET_REQUIRE(opt->conf_floor >= 0.f && opt->conf_floor <= 1.f, "distill_fwd_bwd: conf_floor must lie in [0, 1]");
  SQDET_REQUIRE((preds_dtype == SQDET_F32 || preds_dtype == SQDET_F16) && (teacher_dtype == SQDET_F32 || teacher_dtype == SQDET_F16),
                "distill_fwd_bwd: bad dtype");
  const bool half = preds_dtype == SQDET_F16, thalf = teacher_dtype == SQDET_F16;
  SQDET_REQUIRE(!half || (dpreds_scaled_f16 && loss_scale > 0.f), "distill_fwd_bwd: float16 preds need dpreds_scaled_f16 and a loss scale");
  DistillArgs a;
  a.preds = preds; a.teacher = teacher_preds; a.dpreds = dpreds_inout; a.partial = workspace;
  a.g16 = half ? static_cast<f16*>(dpreds_scaled_f16) : nullptr; a.gscale = half ? loss_scale : 1.f;
  a.B = batch; a.cells = gh * gw; a.K = apg; a.C = classes;
  a.Bg = (float)(global_batch > 0 ? global_batch : batch);
  a.BgA = a.Bg * (float)(gh * gw * apg);
  a.T = opt->temperature; a.c_cls = opt->class_coef; a.c_conf = opt->conf_coef; a.c_box = opt->bbox_coef; a.floor = opt->conf_floor;
  const int blocks = launch_blocks((long)batch * gh * gw * apg);
  hipStream_t st = as_stream(stream);
  if (half && thalf) hipLaunchKernelGGL((distill_kernel<f16, f16>), dim3(blocks), dim3(256), 0, st, a);
  else if (half) hipLaunchKernelGGL((distill_kernel<f16, float>), dim3(blocks), dim3(256), 0, st, a);
  else if (thalf) hipLaunchKernelGGL((distill_kernel<float, f16>), dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((distill_kernel<float, float>), dim3(blocks), dim3(256), 0, st, a);
  SQDET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, workspace, distill3, blocks);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}
