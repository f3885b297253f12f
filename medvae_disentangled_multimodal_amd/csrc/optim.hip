// Fused optimizer step over ONE flat fp32 parameter/gradient/moment buffer (multi-tensor):
//   on_before_optimizer_step: a tensor with any non-finite gradient has its whole grad zeroed
//       (lightning_module.py:468-477, per tensor, no host sync: flags stay on the device)
//   configure_gradient_clipping: global L2 norm clip, coef = min(max_norm/(norm+1e-6), 1)
//       (lightning_module.py:452-466 -> torch.nn.utils.clip_grad_norm_)
//   configure_optimizers: Adam (L2 weight decay) / AdamW (decoupled) with per-tensor step counts
//       (lightning_module.py:390-408 -> torch.optim single-tensor arithmetic)
// Tensors whose gradient is absent this step (`used[t] == 0`, e.g. heads of modalities that are
// not in the batch) are skipped exactly like torch skips params with grad None.
//
// mvae_multi_tensor_adam_ema: the same three launches, the third also keeping an exponential moving average of the
// weights (the reference's exponential_moving_average helper, src/utils/training_utils.py:221-227:
// ema.mul_(decay).add_(param, alpha=1 - decay) over ALL parameters) in a flat buffer laid out like the parameters:
// after p has its new value, ema = ema * d + omd * p -- one more read and one more write per element (36 instead of
// 28 B/param) in the pass that already holds p in registers. A tensor without a gradient this step skips Adam and
// still averages. mvae_swap_buffers exchanges two flat buffers in place (the averaged weights under the model).
#include "common.h"

namespace mvae {

struct MtArgs {
  float* p; float* g; float* m; float* v;
  const int* chunk_tensor; const long long* chunk_start; const int* chunk_len;
  const int* tensor_chunk_begin;  // [T+1]
  const int* used; int* step; int* bad;
  double* chunk_sumsq; int* chunk_bad;
  float* scalars;  // [0] total norm, [1] clip coef
  int T, nchunks;
  float gscale;
};

__global__ void __launch_bounds__(256) mt_chunk_stats_kernel(MtArgs a) {
  __shared__ double sh[4];
  __shared__ int shb[4];
  const int ch = blockIdx.x;
  const long long s = a.chunk_start[ch];
  const int len = a.chunk_len[ch];
  double acc = 0;
  int badf = 0;
  const int body = (s & 3) == 0 ? (len & ~3) : 0;
  for (int i = threadIdx.x * 4; i < body; i += blockDim.x * 4) {
    const float4 g4 = *(const float4*)(a.g + s + i);
    const float xs[4] = {g4.x * a.gscale, g4.y * a.gscale, g4.z * a.gscale, g4.w * a.gscale};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!isfinite(xs[e])) badf = 1;
      acc += (double)xs[e] * xs[e];
    }
  }
  for (int i = body + threadIdx.x; i < len; i += blockDim.x) {
    const float x = a.g[s + i] * a.gscale;
    if (!isfinite(x)) badf = 1;
    acc += (double)x * x;
  }
  acc = wave_sum_d(acc);
  badf = __any(badf) ? 1 : 0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sh[w] = acc; shb[w] = badf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0;
    int b = 0;
    for (int i = 0; i < 4; ++i) { t += sh[i]; b |= shb[i]; }
    a.chunk_sumsq[ch] = t;
    a.chunk_bad[ch] = b;
  }
}

__global__ void __launch_bounds__(256) mt_finalize_kernel(MtArgs a, float max_norm, int do_clip) {
  __shared__ double sh[4];
  double acc = 0;
  for (int t = threadIdx.x; t < a.T; t += blockDim.x) {
    double s = 0;
    int b = 0;
    for (int c = a.tensor_chunk_begin[t]; c < a.tensor_chunk_begin[t + 1]; ++c) {
      s += a.chunk_sumsq[c];
      b |= a.chunk_bad[c];
    }
    a.bad[t] = b;
    if (a.used[t]) {
      a.step[t] += 1;
      if (!b) acc += s;
    }
  }
  acc = wave_sum_d(acc);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = sqrt(sh[0] + sh[1] + sh[2] + sh[3]);
    float coef = 1.f;
    if (do_clip) {
      coef = (float)((double)max_norm / (tot + 1e-6));
      if (coef > 1.f) coef = 1.f;
    }
    a.scalars[0] = (float)tot;
    a.scalars[1] = coef;
  }
}

// w = 1 - beta1 and omb2 = 1 - beta2 come rounded from the double difference, as torch forms them (1 - 0.999 -> 0.001f):
// 1.f - 0.999f is 0.00099998713, 1.3e-5 off, and exp_avg_sq carried that error in every element
// ... and the bias corrections 1 - beta^step from the double betas (torch: Python floats), consistent with them; the
// step size lr / bias_correction1 and the decoupled decay 1 - lr * wd likewise from the double lr and weight decay
// EMA: after p has its new value, ema = ema * d + omd * p with d and omd = 1 - d rounded from the double decay (as w and
// omb2 are); a tensor that is not `used` this step takes that update alone.
template <bool EMA>
__global__ void __launch_bounds__(256) mt_adam_kernel(MtArgs a, double lr, double b1d, double b2d, float eps, double wdd,
                                                      int decoupled, float* ema, double emad) {
  const float b2 = (float)b2d, w = (float)(1.0 - b1d), omb2 = (float)(1.0 - b2d), wd = (float)wdd;
  const float d = (float)emad, omd = (float)(1.0 - emad);
  const int ch = blockIdx.x;
  const int t = a.chunk_tensor[ch];
  const long long s = a.chunk_start[ch];
  const int len = a.chunk_len[ch];
  if (!a.used[t]) {
    if constexpr (EMA) {
      const int body = (s & 3) == 0 ? (len & ~3) : 0;
      for (int i = threadIdx.x * 4; i < body; i += blockDim.x * 4) {
        const long long e = s + i;
        const float4 p4 = *(const float4*)(a.p + e);
        float4 e4 = *(const float4*)(ema + e);
        e4.x = e4.x * d + omd * p4.x;
        e4.y = e4.y * d + omd * p4.y;
        e4.z = e4.z * d + omd * p4.z;
        e4.w = e4.w * d + omd * p4.w;
        *(float4*)(ema + e) = e4;
      }
      for (int i = body + threadIdx.x; i < len; i += blockDim.x) {
        const long long e = s + i;
        ema[e] = ema[e] * d + omd * a.p[e];
      }
    }
    return;
  }
  const bool zero = a.bad[t] != 0;
  const float coef = a.scalars[1];
  const int step = a.step[t];
  const double bc1 = 1.0 - pow(b1d, (double)step);
  const double bc2 = 1.0 - pow(b2d, (double)step);
  const float step_size = (float)(lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  const float decay = (float)(1.0 - lr * wdd);
  // one element of the update (torch.optim.Adam/AdamW single-tensor arithmetic, in its operation order)
  auto upd = [&](float g, float& p, float& m, float& v) -> float {
    g = zero ? 0.f : g * a.gscale;
    g = g * coef;
    const float gout = g;
    if (decoupled) p = p * decay;
    else if (wd != 0.f) g = g + wd * p;
    m = (w < 0.5f) ? m + w * (g - m) : g - (g - m) * (1.f - w);
    v = v * b2 + omb2 * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p + (-step_size) * (m / denom);
    return gout;
  };
  // 16-B body (flat-buffer tensors are 16-B aligned), scalar tail
  const int body = (s & 3) == 0 ? (len & ~3) : 0;
  for (int i = threadIdx.x * 4; i < body; i += blockDim.x * 4) {
    const long long e = s + i;
    float4 g4 = *(const float4*)(a.g + e), p4 = *(const float4*)(a.p + e);
    float4 m4 = *(const float4*)(a.m + e), v4 = *(const float4*)(a.v + e);
    g4.x = upd(g4.x, p4.x, m4.x, v4.x);
    g4.y = upd(g4.y, p4.y, m4.y, v4.y);
    g4.z = upd(g4.z, p4.z, m4.z, v4.z);
    g4.w = upd(g4.w, p4.w, m4.w, v4.w);
    *(float4*)(a.g + e) = g4;
    *(float4*)(a.p + e) = p4;
    *(float4*)(a.m + e) = m4;
    *(float4*)(a.v + e) = v4;
    if constexpr (EMA) {
      float4 e4 = *(const float4*)(ema + e);
      e4.x = e4.x * d + omd * p4.x;
      e4.y = e4.y * d + omd * p4.y;
      e4.z = e4.z * d + omd * p4.z;
      e4.w = e4.w * d + omd * p4.w;
      *(float4*)(ema + e) = e4;
    }
  }
  for (int i = body + threadIdx.x; i < len; i += blockDim.x) {
    const long long e = s + i;
    float g = zero ? 0.f : a.g[e] * a.gscale;
    g = g * coef;
    a.g[e] = g;
    float p = a.p[e];
    if (decoupled) p = p * decay;
    else if (wd != 0.f) g = g + wd * p;
    float m = a.m[e];
    m = (w < 0.5f) ? m + w * (g - m) : g - (g - m) * (1.f - w);
    float v = a.v[e] * b2 + omb2 * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p + (-step_size) * (m / denom);
    a.m[e] = m;
    a.v[e] = v;
    a.p[e] = p;
    if constexpr (EMA) ema[e] = ema[e] * d + omd * p;
  }
}

// a <-> b in place: 16-B loads and stores over a grid-stride loop (both buffers 16-B aligned), scalar tail
__global__ void __launch_bounds__(256) swap_buffers_kernel(float* a, float* b, size_t n, int vec) {
  const size_t body = vec ? (n & ~(size_t)3) : 0;
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < body; i += stride) {
    const float4 x = *(const float4*)(a + i), y = *(const float4*)(b + i);
    *(float4*)(a + i) = y;
    *(float4*)(b + i) = x;
  }
  if (blockIdx.x == 0) {
    for (size_t i = body + threadIdx.x; i < n; i += blockDim.x) {
      const float x = a[i];
      a[i] = b[i];
      b[i] = x;
    }
  }
}

}  // namespace mvae

using namespace mvae;

// the three launches of one step (ema == nullptr: no averaged copy)
static int mt_adam_launch(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int* chunk_tensor,
                          const long long* chunk_start, const int* chunk_len, int nchunks,
                          const int* tensor_chunk_begin, int ntensors, const int* used, int* step, float grad_scale,
                          float max_norm, int do_clip, double lr, double beta1, double beta2, float eps,
                          double weight_decay, int decoupled, void* workspace, size_t workspace_bytes, float* scalars,
                          float* ema, double ema_decay, void* stream) {
  const size_t need = (size_t)nchunks * (sizeof(double) + sizeof(int)) + (size_t)ntensors * sizeof(int) + 64;
  if (nchunks <= 0 || ntensors <= 0) { set_error("adam: empty"); return MVAE_EINVAL; }
  if (workspace_bytes < need) { set_error("adam: workspace too small"); return MVAE_EWORKSPACE; }
  MtArgs a{};
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq;
  a.chunk_tensor = chunk_tensor; a.chunk_start = chunk_start; a.chunk_len = chunk_len;
  a.tensor_chunk_begin = tensor_chunk_begin; a.used = used; a.step = step;
  a.chunk_sumsq = (double*)workspace;
  a.chunk_bad = (int*)((char*)workspace + (size_t)nchunks * sizeof(double));
  a.bad = a.chunk_bad + nchunks;
  a.scalars = scalars; a.T = ntensors; a.nchunks = nchunks; a.gscale = grad_scale;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mt_chunk_stats_kernel, dim3(nchunks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(mt_finalize_kernel, dim3(1), dim3(256), 0, st, a, max_norm, do_clip);
  if (ema)
    hipLaunchKernelGGL(mt_adam_kernel<true>, dim3(nchunks), dim3(256), 0, st, a, lr, beta1, beta2, eps, weight_decay,
                       decoupled, ema, ema_decay);
  else
    hipLaunchKernelGGL(mt_adam_kernel<false>, dim3(nchunks), dim3(256), 0, st, a, lr, beta1, beta2, eps, weight_decay,
                       decoupled, (float*)nullptr, 0.0);
  return launch_status();
}

extern "C" {

// One optimizer step over flat buffers. chunk tables / tensor_chunk_begin describe how the flat
// buffer splits into tensors (host-built once). Workspace: chunk_sumsq (double[nchunks]),
// chunk_bad (int[nchunks]), bad (int[T]); scalars: float[2] out (total norm, clip coef).
int mvae_multi_tensor_adam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int* chunk_tensor,
                           const long long* chunk_start, const int* chunk_len, int nchunks,
                           const int* tensor_chunk_begin, int ntensors, const int* used, int* step, float grad_scale,
                           float max_norm, int do_clip, double lr, double beta1, double beta2, float eps,
                           double weight_decay, int decoupled, void* workspace, size_t workspace_bytes, float* scalars,
                           void* stream) {
  return mt_adam_launch(params, grads, exp_avg, exp_avg_sq, chunk_tensor, chunk_start, chunk_len, nchunks,
                        tensor_chunk_begin, ntensors, used, step, grad_scale, max_norm, do_clip, lr, beta1, beta2, eps,
                        weight_decay, decoupled, workspace, workspace_bytes, scalars, nullptr, 0.0, stream);
}

// The same step, also averaging the weights: ema (laid out like params) = ema * ema_decay + (1 - ema_decay) * params
// after the update, for every tensor (used or not). params, grads, moments, step and scalars come out as above.
int mvae_multi_tensor_adam_ema(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int* chunk_tensor,
                               const long long* chunk_start, const int* chunk_len, int nchunks,
                               const int* tensor_chunk_begin, int ntensors, const int* used, int* step,
                               float grad_scale, float max_norm, int do_clip, double lr, double beta1, double beta2,
                               float eps, double weight_decay, int decoupled, void* workspace, size_t workspace_bytes,
                               float* scalars, float* ema, double ema_decay, void* stream) {
  if (!ema) { set_error("adam_ema: null ema buffer"); return MVAE_EINVAL; }
  if (!(ema_decay >= 0.0 && ema_decay < 1.0)) { set_error("adam_ema: ema_decay must be in [0, 1)"); return MVAE_EINVAL; }
  return mt_adam_launch(params, grads, exp_avg, exp_avg_sq, chunk_tensor, chunk_start, chunk_len, nchunks,
                        tensor_chunk_begin, ntensors, used, step, grad_scale, max_norm, do_clip, lr, beta1, beta2, eps,
                        weight_decay, decoupled, workspace, workspace_bytes, scalars, ema, ema_decay, stream);
}

// Exchange two device buffers of n floats in place (no temporary).
int mvae_swap_buffers(float* a, float* b, size_t n, void* stream) {
  if (!a || !b || n == 0) { set_error("swap_buffers: null pointer or empty"); return MVAE_EINVAL; }
  if (a == b) return MVAE_OK;
  const int vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  const size_t groups = (n + 1023) / 1024;  // 256 threads x 4 floats
  const int blocks = (int)(groups < 2048 ? groups : 2048);
  hipLaunchKernelGGL(swap_buffers_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, b, n, vec);
  return launch_status();
}

size_t mvae_multi_tensor_adam_workspace_bytes(int nchunks, int ntensors) {
  return (size_t)nchunks * (sizeof(double) + sizeof(int)) + (size_t)ntensors * sizeof(int) + 64;
}

}  // extern "C"
