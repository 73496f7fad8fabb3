// The training step's optimizer for gfx950: Momentum update with per-variable clip_by_norm and weight decay (reference
// src/nn_skeleton.py:329-361; sqdet_optimizer_step), and the same three passes with options -- Nesterov / AdamW, a global clip, an
// EMA of the weights (sqdet_optimizer_step_opt).  One kernel for pass 1 and one for pass 2 under both entry points;
// pass 3 has a vector form for the rules and keeps the reference's scalar form for sqdet_optimizer_step.
// Compiled with -ffp-contract=off: every element-wise operator is one float32 IEEE operation in the order written.
#include <math.h>

#include <vector>

#include "common.h"

namespace sqdet {

// Segment table: variable v occupies [seg[v].off, +count) of the flat parameter / gradient / momentum
// buffers.  Pass 1 adds the weight-decay gradient and writes per-block partial sums of squares; pass 2
// (one block) finishes the norms in a fixed order; pass 3 clips and applies the rule.
struct OptSeg { long off; long count; float decay; int first_block; int nblocks; };

// Pass 1.  COUPLE: the decay goes onto the gradient (not under AdamW, whose decay is decoupled; same partition, same order).
template <bool COUPLE>
__global__ __launch_bounds__(256) void opt_sumsq_kernel(const OptSeg* __restrict__ segs, const int* __restrict__ block_seg,
                                                        const float* __restrict__ w, float* __restrict__ g,
                                                        double* __restrict__ partial, float grad_scale) {
  __shared__ double red[256];
  const int v = block_seg[blockIdx.x];
  const OptSeg s = segs[v];
  const int lb = blockIdx.x - s.first_block;
  double acc = 0.0;
  for (long i = (long)lb * 256 + threadIdx.x; i < s.count; i += (long)s.nblocks * 256) {
    float gi = g[s.off + i] * grad_scale;   // grad_scale = 1/world_size after a SUM all-reduce
    if (COUPLE && s.decay != 0.f) gi = gi + s.decay * w[s.off + i];
    g[s.off + i] = gi;
    acc += (double)gi * (double)gi;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// Pass 2 (one block of 256): the clip factors, the overflow flag of mixed-precision training (a non-finite gradient norm in ANY
// variable: flag[0] = 1 and pass 3 leaves every buffer untouched) and -- state != NULL, on a step that applies -- the device state
// state[0..3) = (t, beta1^t, beta2^t) advanced by one update and the three float32 scalars pass 3 reads,
// derived[0..3) = (1 / (1 - beta1^t), 1 / (1 - beta2^t), 1 - d), each formed in float64 and rounded once (the first two under AdamW,
// the third with an EMA: nothing else reads them).  Global clip: the
// per-variable float64 sums are added in variable-index order (laps of 256 through LDS, one thread adding).
__global__ __launch_bounds__(256) void opt_norm_kernel(const OptSeg* __restrict__ segs, const double* __restrict__ partial,
                                                       float* __restrict__ scale, int nvars, float max_norm, int global_clip,
                                                       int adamw, double beta1, double beta2, double ema_decay, int ema_warmup,
                                                       double* __restrict__ state, float* __restrict__ derived,
                                                       int* __restrict__ flag, int* __restrict__ found_inf) {
  __shared__ double vsum[256];
  __shared__ float gfactor;
  int bad = 0;
  double S = 0.0;                                   // (thread 0)
  for (int base = 0; base < nvars; base += 256) {   // uniform trip count: the barriers below are reached by every thread
    const int v = base + threadIdx.x;
    if (v < nvars) {
      double s = 0.0;
      for (int b = 0; b < segs[v].nblocks; ++b) s += partial[segs[v].first_block + b];
      const float nrm = (float)sqrt(s);
      if (!(nrm <= 3.0e38f)) bad = 1;               // inf or NaN
      if (!global_clip) scale[v] = max_norm / fmaxf(nrm, max_norm);   // tf.clip_by_norm: g * clip / max(||g||, clip)
      vsum[threadIdx.x] = s;
    }
    if (global_clip) {
      __syncthreads();
      if (threadIdx.x == 0) {
        const int n = nvars - base < 256 ? nvars - base : 256;
        for (int k = 0; k < n; ++k) S += vsum[k];
      }
      __syncthreads();
    }
  }
  if (global_clip) {
    if (threadIdx.x == 0) {
      const float N = (float)sqrt(S);               // tf.clip_by_global_norm: every g * clip / max(||all g||, clip)
      if (!(N <= 3.0e38f)) bad = 1;
      gfactor = max_norm / fmaxf(N, max_norm);
    }
    __syncthreads();
    const float f = gfactor;
    for (int v = threadIdx.x; v < nvars; v += 256) scale[v] = f;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    flag[0] = bad;
    if (found_inf) found_inf[0] = bad;
    if (!bad && state) {                            // a skipped step leaves the state where it was
      const double t = state[0] + 1.0, p1 = state[1] * beta1, p2 = state[2] * beta2;
      if (adamw) {                                  // (read by no other rule: two float64 divisions on one thread spared)
        derived[0] = (float)(1.0 / (1.0 - p1));
        derived[1] = (float)(1.0 / (1.0 - p2));
      }
      if (ema_decay > 0.0) {
        double d = ema_decay;
        if (ema_warmup) { const double dw = (1.0 + t) / (10.0 + t); d = dw < d ? dw : d; }
        derived[2] = (float)(1.0 - d);
      }
      state[0] = t; state[1] = p1; state[2] = p2;
    }
  }
}

enum { OPT_RULE_MOMENTUM = 0, OPT_RULE_NESTEROV = 1, OPT_RULE_ADAMW = 2 };
struct OptApplyArgs {
  const OptSeg* segs; const int* block_seg;
  float* w; const float* g; float* a; float* a2; float* e;
  const float* scale; const float* derived; const int* flag;
  float lr, mom, b1, b2, omb1, omb2, eps;   // omb1 = (float)(1 - beta1), omb2 = (float)(1 - beta2): rounded once, on the host
  int vec_ok;                               // every base pointer in use is 16-byte aligned
};
struct OptStepConst { float sc, decay, c1, c2, om; };

// One element; the vector and the scalar path both run exactly this, one rounding per operator in the order written.
template <int RULE, bool EMA>
__device__ __forceinline__ void opt_update(const OptApplyArgs& p, const OptStepConst& k, float& w, float g, float& a, float& a2,
                                           float& e) {
  const float gc = g * k.sc;
  if (RULE == OPT_RULE_ADAMW) {
    a = p.b1 * a + p.omb1 * gc;
    a2 = p.b2 * a2 + p.omb2 * (gc * gc);
    float u = (a * k.c1) / (sqrtf(a2 * k.c2) + p.eps);
    if (k.decay != 0.f) u = u + k.decay * w;        // decoupled: on the update, not on the gradient
    w = w - p.lr * u;
  } else {
    a = p.mom * a + gc;                             // MomentumOptimizer: accum = m*accum + g ; var -= lr*accum
    if (RULE == OPT_RULE_NESTEROV) w = w - p.lr * (gc + p.mom * a);
    else w = w - p.lr * a;
  }
  if (EMA) e = e + k.om * (w - e);                   // on the value just written
}

template <int RULE, bool EMA>
__device__ __forceinline__ void opt_update_at(const OptApplyArgs& p, const OptStepConst& k, long at) {   // the scalar path's element
  float wi = p.w[at], ai = p.a[at], mi = RULE == OPT_RULE_ADAMW ? p.a2[at] : 0.f, ei = EMA ? p.e[at] : 0.f;
  opt_update<RULE, EMA>(p, k, wi, p.g[at], ai, mi, ei);
  p.w[at] = wi; p.a[at] = ai;
  if (RULE == OPT_RULE_ADAMW) p.a2[at] = mi;
  if (EMA) p.e[at] = ei;
}

// Pass 3.
template <int RULE, bool EMA>
__global__ __launch_bounds__(256) void opt_apply_kernel(const OptApplyArgs p) {
  if (p.flag[0]) return;   // overflowed step: skipped, in all five buffers
  const int v = p.block_seg[blockIdx.x];
  const OptSeg s = p.segs[v];
  const int lb = blockIdx.x - s.first_block;
  OptStepConst k;
  k.sc = p.scale[v]; k.decay = s.decay;
  k.c1 = RULE == OPT_RULE_ADAMW ? p.derived[0] : 1.f;
  k.c2 = RULE == OPT_RULE_ADAMW ? p.derived[1] : 1.f;
  k.om = EMA ? p.derived[2] : 0.f;
  const long stride = (long)s.nblocks * 256;
  if (p.vec_ok && (s.off & 3) == 0) {
    // 16-byte vectors, never past the segment's end.  A block keeps pass 1's elements -- the 256-element chunks lb*256 + k*stride --
    // so the gradient it wrote there (and the w this pass leaves for the next step's pass 1) is met in its own XCD's L2: with
    // another assignment pass 1 behind this pass took 21.5 us instead of 11.9 on SqueezeDet's table.  Wave `sub` of the block
    // takes the chunks k = sub, sub + 4, ...: one KiB per wave, array and trip.
    const int sub = threadIdx.x >> 6, lane4 = (threadIdx.x & 63) << 2;
    for (long base = (long)lb * 256 + (long)sub * stride; base < s.count; base += 4 * stride) {
      const long i0 = base + lane4;
      if (i0 + 3 >= s.count) {                      // the segment's last 1 .. 3 elements (or none)
        for (long i = i0; i < s.count; ++i) opt_update_at<RULE, EMA>(p, k, s.off + i);
        continue;
      }
      const long at = s.off + i0;
      f32x4 w4 = *reinterpret_cast<const f32x4*>(p.w + at), a4 = *reinterpret_cast<const f32x4*>(p.a + at), m4 = {0.f, 0.f, 0.f, 0.f},
            e4 = {0.f, 0.f, 0.f, 0.f};
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(p.g + at);
      if (RULE == OPT_RULE_ADAMW) m4 = *reinterpret_cast<const f32x4*>(p.a2 + at);
      if (EMA) e4 = *reinterpret_cast<const f32x4*>(p.e + at);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float wj = w4[j], aj = a4[j], mj = m4[j], ej = e4[j];
        opt_update<RULE, EMA>(p, k, wj, g4[j], aj, mj, ej);
        w4[j] = wj; a4[j] = aj; m4[j] = mj; e4[j] = ej;
      }
      *reinterpret_cast<f32x4*>(p.w + at) = w4;
      *reinterpret_cast<f32x4*>(p.a + at) = a4;
      if (RULE == OPT_RULE_ADAMW) *reinterpret_cast<f32x4*>(p.a2 + at) = m4;
      if (EMA) *reinterpret_cast<f32x4*>(p.e + at) = e4;
    }
    return;
  }
  for (long i = (long)lb * 256 + threadIdx.x; i < s.count; i += stride) opt_update_at<RULE, EMA>(p, k, s.off + i);   // odd offsets, unaligned bases
}

// Pass 3 of sqdet_optimizer_step: the scalar loop of opt_apply_kernel<OPT_RULE_MOMENTUM, false>, the same bits
// (tests/test_gpu_optimizer_options.py asserts it).  It stays beside the vector form because on ResNet50+ConvDet's table (59
// variables, 7.76 M elements) the vector form made the step 0.9 us slower, and this entry is the path of a run without flags
// (DESIGN.md 3.18).
__global__ __launch_bounds__(256) void opt_apply_scalar_kernel(const OptSeg* __restrict__ segs, const int* __restrict__ block_seg,
                                                               float* __restrict__ w, const float* __restrict__ g,
                                                               float* __restrict__ accum, const float* __restrict__ scale,
                                                               float lr, float momentum, const int* __restrict__ flag) {
  if (flag[0]) return;   // overflowed step: skipped
  const int v = block_seg[blockIdx.x];
  const OptSeg s = segs[v];
  const int lb = blockIdx.x - s.first_block;
  const float sc = scale[v];
  for (long i = (long)lb * 256 + threadIdx.x; i < s.count; i += (long)s.nblocks * 256) {
    const float gc = g[s.off + i] * sc;
    const float ac = momentum * accum[s.off + i] + gc;   // MomentumOptimizer: accum = m*accum + g ; var -= lr*accum
    accum[s.off + i] = ac;
    w[s.off + i] = w[s.off + i] - lr * ac;
  }
}

}  // namespace sqdet

using namespace sqdet;

// ---- host side: the segment table lives in a small opaque object ----
struct sqdet_optimizer {
  std::vector<OptSeg> segs;
  std::vector<int> block_seg;
  int nblocks = 0;
};

extern "C" int sqdet_optimizer_create(sqdet_optimizer** out, const long* offsets, const long* counts, const float* decays,
                                      int nvars) {
  SQDET_REQUIRE(out && offsets && counts && decays && nvars > 0, "optimizer_create: bad arguments");
  sqdet_optimizer* o = new sqdet_optimizer();
  for (int v = 0; v < nvars; ++v) {
    OptSeg s;
    s.off = offsets[v]; s.count = counts[v]; s.decay = decays[v];
    long nb = (counts[v] + 256 * 8 - 1) / (256 * 8);
    if (nb < 1) nb = 1;
    if (nb > 64) nb = 64;
    s.first_block = o->nblocks; s.nblocks = (int)nb;
    o->nblocks += (int)nb;
    for (long b = 0; b < nb; ++b) o->block_seg.push_back(v);
    o->segs.push_back(s);
  }
  *out = o;
  return SQDET_OK;
}

extern "C" void sqdet_optimizer_destroy(sqdet_optimizer* o) { delete o; }

// The workspace: segs | block_seg | partial (double) | scale, each part on a multiple of 256 bytes; the flag word and the three
// derived float32 scalars follow the last clip factor, inside the 256 spare bytes.
struct OptWorkspace {
  OptSeg* segs; int* block_seg; double* partial; float* scale; int* flag; float* derived;
  size_t bytes;
  OptWorkspace(const sqdet_optimizer* o, void* base) {
    size_t off = 0;
    auto take = [&](size_t n) {
      char* p = reinterpret_cast<char*>(reinterpret_cast<uintptr_t>(base) + off);
      off = (off + n + 255) / 256 * 256;
      return p;
    };
    segs = reinterpret_cast<OptSeg*>(take(o->segs.size() * sizeof(OptSeg)));
    block_seg = reinterpret_cast<int*>(take(o->block_seg.size() * sizeof(int)));
    partial = reinterpret_cast<double*>(take((size_t)o->nblocks * sizeof(double)));
    bytes = off + o->segs.size() * sizeof(float) + 256;
    scale = reinterpret_cast<float*>(take(o->segs.size() * sizeof(float)));
    flag = reinterpret_cast<int*>(scale + o->segs.size());
    derived = reinterpret_cast<float*>(flag + 1);
  }
};

extern "C" size_t sqdet_optimizer_workspace_bytes(const sqdet_optimizer* o) { return o ? OptWorkspace(o, nullptr).bytes : 0; }

// What an optimizer entry point was called with: the two entries validate, fill one and hand it to optimizer_step_impl.
struct OptStep {
  float *params, *grads, *accum, *accum2, *ema;      // accum2 / ema: NULL where the rule / the options do not use them
  double* state;                                     // NULL: sqdet_optimizer_step, which keeps none and takes the scalar pass 3
  void* workspace;
  float lr, max_grad_norm, grad_scale;
  sqdet_optimizer_options_t opt;
  int32_t* found_inf;
  sqdet_stream_t stream;
};

template <int RULE>
static void launch_opt_apply(bool ema, int nblocks, hipStream_t st, const OptApplyArgs& p) {
  if (ema) hipLaunchKernelGGL((opt_apply_kernel<RULE, true>), dim3(nblocks), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((opt_apply_kernel<RULE, false>), dim3(nblocks), dim3(256), 0, st, p);
}

static int optimizer_step_impl(const sqdet_optimizer* o, const OptStep& c) {
  const sqdet_optimizer_options_t& opt = c.opt;
  const bool adamw = opt.rule == OPT_RULE_ADAMW, use_ema = opt.ema_decay > 0.0;
  hipStream_t st = as_stream(c.stream);
  const OptWorkspace ws(o, c.workspace);
  const int nvars = (int)o->segs.size();
  SQDET_CHECK_HIP(hipMemcpyAsync(ws.segs, o->segs.data(), o->segs.size() * sizeof(OptSeg), hipMemcpyHostToDevice, st));
  SQDET_CHECK_HIP(hipMemcpyAsync(ws.block_seg, o->block_seg.data(), o->block_seg.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (adamw)
    hipLaunchKernelGGL((opt_sumsq_kernel<false>), dim3(o->nblocks), dim3(256), 0, st, ws.segs, ws.block_seg, c.params, c.grads, ws.partial, c.grad_scale);
  else
    hipLaunchKernelGGL((opt_sumsq_kernel<true>), dim3(o->nblocks), dim3(256), 0, st, ws.segs, ws.block_seg, c.params, c.grads, ws.partial, c.grad_scale);
  SQDET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(opt_norm_kernel, dim3(1), dim3(256), 0, st, ws.segs, ws.partial, ws.scale, nvars, c.max_grad_norm, opt.clip,
                     adamw ? 1 : 0, (double)opt.beta1, (double)opt.beta2, use_ema ? opt.ema_decay : 0.0, opt.ema_warmup != 0, c.state,
                     ws.derived, ws.flag, c.found_inf);
  SQDET_CHECK_HIP(hipGetLastError());
  if (!c.state) {
    hipLaunchKernelGGL(opt_apply_scalar_kernel, dim3(o->nblocks), dim3(256), 0, st, ws.segs, ws.block_seg, c.params, c.grads, c.accum,
                       ws.scale, c.lr, opt.momentum, ws.flag);
    SQDET_CHECK_HIP(hipGetLastError());
    return SQDET_OK;
  }
  OptApplyArgs p;
  p.segs = ws.segs; p.block_seg = ws.block_seg;
  p.w = c.params; p.g = c.grads; p.a = c.accum; p.a2 = adamw ? c.accum2 : nullptr; p.e = use_ema ? c.ema : nullptr;
  p.scale = ws.scale; p.derived = ws.derived; p.flag = ws.flag;
  p.lr = c.lr; p.mom = opt.momentum; p.b1 = opt.beta1; p.b2 = opt.beta2; p.eps = opt.eps;
  p.omb1 = (float)(1.0 - (double)opt.beta1); p.omb2 = (float)(1.0 - (double)opt.beta2);
  uintptr_t bits = reinterpret_cast<uintptr_t>(c.params) | reinterpret_cast<uintptr_t>(c.grads) | reinterpret_cast<uintptr_t>(c.accum);
  if (adamw) bits |= reinterpret_cast<uintptr_t>(c.accum2);
  if (use_ema) bits |= reinterpret_cast<uintptr_t>(c.ema);
  p.vec_ok = (bits & 15) == 0;
  if (opt.rule == OPT_RULE_MOMENTUM) launch_opt_apply<OPT_RULE_MOMENTUM>(use_ema, o->nblocks, st, p);
  else if (opt.rule == OPT_RULE_NESTEROV) launch_opt_apply<OPT_RULE_NESTEROV>(use_ema, o->nblocks, st, p);
  else launch_opt_apply<OPT_RULE_ADAMW>(use_ema, o->nblocks, st, p);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

// The reference's update: Momentum, the per-variable clip, no EMA, no device state.
extern "C" int sqdet_optimizer_step(sqdet_optimizer* o, float* params, float* grads, float* accum, void* workspace,
                                    float lr, float momentum, float max_grad_norm, float grad_scale, int32_t* found_inf,
                                    sqdet_stream_t stream) {
  SQDET_REQUIRE(o && params && grads && accum && workspace, "optimizer_step: null pointer");
  const OptStep c = {params, grads, accum, nullptr, nullptr, nullptr, workspace, lr, max_grad_norm, grad_scale,
                     {OPT_RULE_MOMENTUM, SQDET_CLIP_PER_VARIABLE, momentum, 0.f, 0.f, 0.f, 0.0, 0}, found_inf, stream};
  return optimizer_step_impl(o, c);
}

extern "C" int sqdet_optimizer_step_opt(sqdet_optimizer* o, float* params, float* grads, float* accum, float* accum2, float* ema,
                                        double* state, void* workspace, float lr, float max_grad_norm, float grad_scale,
                                        const sqdet_optimizer_options_t* opt, int32_t* found_inf, sqdet_stream_t stream) {
  SQDET_REQUIRE(o && params && grads && accum && state && workspace && opt, "optimizer_step_opt: null pointer");
  SQDET_REQUIRE(opt->rule >= OPT_RULE_MOMENTUM && opt->rule <= OPT_RULE_ADAMW, "optimizer_step_opt: rule must be 0 (momentum), 1 (nesterov) or 2 (adamw)");
  SQDET_REQUIRE(opt->clip == 0 || opt->clip == 1, "optimizer_step_opt: clip must be 0 (per variable) or 1 (global)");
  SQDET_REQUIRE(opt->momentum >= 0.f && opt->momentum < 1.f, "optimizer_step_opt: momentum must lie in [0, 1)");
  SQDET_REQUIRE(opt->beta1 >= 0.f && opt->beta1 < 1.f && opt->beta2 >= 0.f && opt->beta2 < 1.f, "optimizer_step_opt: beta1 and beta2 must lie in [0, 1)");
  SQDET_REQUIRE(opt->eps > 0.f && opt->eps <= 3.0e38f, "optimizer_step_opt: eps must be finite and positive");
  SQDET_REQUIRE(opt->ema_decay >= 0.0 && opt->ema_decay < 1.0, "optimizer_step_opt: ema_decay must lie in [0, 1)");
  SQDET_REQUIRE(opt->rule != OPT_RULE_ADAMW || accum2, "optimizer_step_opt: adamw needs accum2");
  SQDET_REQUIRE(!(opt->ema_decay > 0.0) || ema, "optimizer_step_opt: ema_decay > 0 needs the ema buffer");
  for (const OptSeg& s : o->segs)
    SQDET_REQUIRE(s.decay >= 0.f && s.decay <= 3.0e38f, "optimizer_step_opt: a variable's decay must be finite and >= 0");
  const OptStep c = {params, grads, accum, accum2, ema, state, workspace, lr, max_grad_norm, grad_scale, *opt, found_inf, stream};
  return optimizer_step_impl(o, c);
}
