// Linear attention core (LinearAttention / LinAttnBlock, src/models/encoder_decoder.py:36-65, heads = 1): the memory-bound
// stages around the four batched GEMMs of ops.LinAttnCoreFn. q, k, v are the channel slices [0:C], [C:2C], [2C:3C] of one
// NHWC tensor [batch][n][3C] and are read in place through its leading dimension.
//   kstats   : per (image, channel) max m and 1 / sum_n exp(k - m) over the n tokens -- a column reduction: lanes run
//              across channels (16-B loads), token rows across the rest of the workgroup and across workgroups; the
//              (max, sum) pairs are merged in a fixed order (LDS tree, then the splits in sequence): no atomics
//   ksoftmax : ksm [batch][n][C] = exp(k - m) / Z, the compact GEMM operand (scratch, recomputed in the backward)
//   dk       : dk = ksm o (dksm - r) in place over the k slice of the gradient tensor, which holds dksm = V dctx^T on
//              entry; ksm is recomputed from k, m, 1/Z on load. r[d] = sum_n ksm[n][d] dksm[n][d] is the column dot of
//              the dksm actually computed (a reduction pass shaped like kstats), not sum_e dctx[d][e] ctx[d][e] from
//              the two C x C matrices: the two are equal in exact arithmetic, but dksm - r cancels (to exactly 0 for
//              one token) only when r carries the same rounding as dksm, whatever the GEMM arithmetic
// Everything is fp32 with expf; nothing of size n x n exists.
#include "common.h"

#include <math.h>

#include <algorithm>

namespace mvae {

constexpr int LA_NT = 256;         // threads per workgroup: tc channel quads x (256 / tc) token rows
constexpr int LA_MAX_SPLITS = 64;  // token splits of the statistics pass
constexpr int LA_MIN_TOKENS = 64;  // tokens per split at least
constexpr int LA_BLOCKS = 2048;    // workgroups a streaming launch aims for

struct LaTile {
  int tc_log2, rows, cgroups;
};

// lanes across channels: the smallest power of two covering C / 4 quads, 64 at most (1 KiB per wave and row)
static LaTile la_tile(int c) {
  const int quads = c >> 2;
  int l = 0;
  while ((1 << l) < quads && l < 6) ++l;
  return LaTile{l, LA_NT >> l, cdiv(quads, 1 << l)};
}

// tokens per split and the split count of the statistics pass (no split is empty)
static void la_splits(int batch, int n, int c, int* per, int* splits) {
  const LaTile t = la_tile(c);
  const long long want = cdiv(LA_BLOCKS / 2, (long long)t.cgroups * batch);
  const long long cap = std::max(1, n / LA_MIN_TOKENS);
  const int s = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(want, cap), LA_MAX_SPLITS));
  *per = cdiv(n, s);
  *splits = cdiv(n, *per);
}

__device__ __forceinline__ void la_update(float& m, float& s, float x) {
  // running (max, sum of exp(. - max)): one exp per element
  if (x <= m) {
    s += expf(x - m);
  } else {
    s = s * expf(m - x) + 1.f;
    m = x;
  }
}

__device__ __forceinline__ void la_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  // (an empty partial is (-inf, 0): its factor is taken as 1 so that -inf - -inf never forms)
  const float e1 = m == mm ? 1.f : expf(m - mm), e2 = m2 == mm ? 1.f : expf(m2 - mm);
  s = s * e1 + s2 * e2;
  m = mm;
}

// grid (channel groups, splits, batch). final: out = stats [batch][2][C] (m, 1/Z); else out = partials
// [batch][splits][2][C] (m, sum)
__global__ void __launch_bounds__(LA_NT) linattn_kstats_kernel(const float* __restrict__ k, long long ldk, long long sk,
                                                               float* __restrict__ out, int n, int c, int tc_log2,
                                                               int per, int final) {
  __shared__ float4 sm[LA_NT], ss[LA_NT];
  const int tid = threadIdx.x, tc = 1 << tc_log2, rows = LA_NT >> tc_log2;
  const int tx = tid & (tc - 1), ty = tid >> tc_log2;
  const int q = blockIdx.x * tc + tx;
  const int b = blockIdx.z, sp = blockIdx.y;
  const int t0 = sp * per, t1 = min(n, t0 + per);
  const bool live = q * 4 < c;
  float4 m{-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s{0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float* p = k + b * sk + q * 4;
#pragma unroll 4
    for (int t = t0 + ty; t < t1; t += rows) {
      const float4 v = *reinterpret_cast<const float4*>(p + (long long)t * ldk);
      la_update(m.x, s.x, v.x);
      la_update(m.y, s.y, v.y);
      la_update(m.z, s.z, v.z);
      la_update(m.w, s.w, v.w);
    }
  }
  sm[tid] = m;
  ss[tid] = s;
  __syncthreads();
  for (int h = rows >> 1; h >= 1; h >>= 1) {  // fixed-order tree over the token rows
    if (ty < h) {
      const float4 m2 = sm[tid + (h << tc_log2)], s2 = ss[tid + (h << tc_log2)];
      la_merge(m.x, s.x, m2.x, s2.x);
      la_merge(m.y, s.y, m2.y, s2.y);
      la_merge(m.z, s.z, m2.z, s2.z);
      la_merge(m.w, s.w, m2.w, s2.w);
      sm[tid] = m;
      ss[tid] = s;
    }
    __syncthreads();
  }
  if (ty == 0 && live) {
    if (final) {
      float* o = out + (long long)b * 2 * c + q * 4;
      *reinterpret_cast<float4*>(o) = m;
      *reinterpret_cast<float4*>(o + c) = float4{1.f / s.x, 1.f / s.y, 1.f / s.z, 1.f / s.w};
    } else {
      float* o = out + ((long long)b * gridDim.y + sp) * 2 * c + q * 4;
      *reinterpret_cast<float4*>(o) = m;
      *reinterpret_cast<float4*>(o + c) = s;
    }
  }
}

// partials [batch][splits][2][C] -> stats [batch][2][C], the splits in sequence; one thread per (image, channel quad)
__global__ void __launch_bounds__(LA_NT) linattn_kstats_merge_kernel(const float* __restrict__ part,
                                                                     float* __restrict__ stats, int batch, int c,
                                                                     int splits) {
  const int quads = c >> 2;
  const int e = blockIdx.x * LA_NT + threadIdx.x;
  if (e >= batch * quads) return;
  const int b = e / quads, q = e - b * quads;
  const float* p = part + (long long)b * splits * 2 * c + q * 4;
  float4 m = *reinterpret_cast<const float4*>(p), s = *reinterpret_cast<const float4*>(p + c);
  for (int z = 1; z < splits; ++z) {
    const float4 m2 = *reinterpret_cast<const float4*>(p + (long long)z * 2 * c);
    const float4 s2 = *reinterpret_cast<const float4*>(p + (long long)z * 2 * c + c);
    la_merge(m.x, s.x, m2.x, s2.x);
    la_merge(m.y, s.y, m2.y, s2.y);
    la_merge(m.z, s.z, m2.z, s2.z);
    la_merge(m.w, s.w, m2.w, s2.w);
  }
  float* o = stats + (long long)b * 2 * c + q * 4;
  *reinterpret_cast<float4*>(o) = m;
  *reinterpret_cast<float4*>(o + c) = float4{1.f / s.x, 1.f / s.y, 1.f / s.z, 1.f / s.w};
}

__device__ __forceinline__ float4 la_ksm(float4 kv, float4 m, float4 rz) {
  return float4{expf(kv.x - m.x) * rz.x, expf(kv.y - m.y) * rz.y, expf(kv.z - m.z) * rz.z, expf(kv.w - m.w) * rz.w};
}

// grid (channel groups, row blocks, batch); DK = 0: ksm = softmax(k) written compact; DK = 1: g (the k slice of the
// gradient, holding dksm) <- ksm o (g - r)
template <int DK>
__global__ void __launch_bounds__(LA_NT) linattn_apply_kernel(const float* __restrict__ k, long long ldk, long long sk,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ r, float* g, long long ldg,
                                                              long long sg, int n, int c, int tc_log2) {
  const int tid = threadIdx.x, tc = 1 << tc_log2, rows = LA_NT >> tc_log2;
  const int tx = tid & (tc - 1), ty = tid >> tc_log2;
  const int q = blockIdx.x * tc + tx;
  const int b = blockIdx.z;
  if (q * 4 >= c) return;
  const float* st = stats + (long long)b * 2 * c + q * 4;
  const float4 m = *reinterpret_cast<const float4*>(st), rz = *reinterpret_cast<const float4*>(st + c);
  float4 rr{0.f, 0.f, 0.f, 0.f};
  if constexpr (DK == 1) rr = *reinterpret_cast<const float4*>(r + (long long)b * c + q * 4);
  const float* kp = k + b * sk + q * 4;
  float* gp = g + b * sg + q * 4;
#pragma unroll 4
  for (int t = blockIdx.y * rows + ty; t < n; t += gridDim.y * rows) {
    const float4 p = la_ksm(*reinterpret_cast<const float4*>(kp + (long long)t * ldk), m, rz);
    float4* o = reinterpret_cast<float4*>(gp + (long long)t * ldg);
    if constexpr (DK == 1) {
      const float4 d = *o;
      *o = float4{p.x * (d.x - rr.x), p.y * (d.y - rr.y), p.z * (d.z - rr.z), p.w * (d.w - rr.w)};
    } else {
      *o = p;
    }
  }
}

// grid (channel groups, splits, batch): r = sum over the tokens of ksm o g (g = the k slice of the gradient holding
// dksm), ksm recomputed from k and stats. final: out = r [batch][C]; else out = partials [batch][splits][C]
__global__ void __launch_bounds__(LA_NT) linattn_coldot_kernel(const float* __restrict__ k, long long ldk, long long sk,
                                                               const float* __restrict__ stats,
                                                               const float* __restrict__ g, long long ldg, long long sg,
                                                               float* __restrict__ out, int n, int c, int tc_log2,
                                                               int per, int final) {
  __shared__ float4 sa[LA_NT];
  const int tid = threadIdx.x, tc = 1 << tc_log2, rows = LA_NT >> tc_log2;
  const int tx = tid & (tc - 1), ty = tid >> tc_log2;
  const int q = blockIdx.x * tc + tx;
  const int b = blockIdx.z, sp = blockIdx.y;
  const int t0 = sp * per, t1 = min(n, t0 + per);
  const bool live = q * 4 < c;
  float4 acc{0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float* st = stats + (long long)b * 2 * c + q * 4;
    const float4 m = *reinterpret_cast<const float4*>(st), rz = *reinterpret_cast<const float4*>(st + c);
    const float* kp = k + b * sk + q * 4;
    const float* gp = g + b * sg + q * 4;
#pragma unroll 4
    for (int t = t0 + ty; t < t1; t += rows) {
      const float4 p = la_ksm(*reinterpret_cast<const float4*>(kp + (long long)t * ldk), m, rz);
      const float4 d = *reinterpret_cast<const float4*>(gp + (long long)t * ldg);
      acc.x += p.x * d.x;
      acc.y += p.y * d.y;
      acc.z += p.z * d.z;
      acc.w += p.w * d.w;
    }
  }
  sa[tid] = acc;
  __syncthreads();
  for (int h = rows >> 1; h >= 1; h >>= 1) {  // fixed-order tree over the token rows
    if (ty < h) {
      const float4 a2 = sa[tid + (h << tc_log2)];
      acc = float4{acc.x + a2.x, acc.y + a2.y, acc.z + a2.z, acc.w + a2.w};
      sa[tid] = acc;
    }
    __syncthreads();
  }
  if (ty == 0 && live) {
    float* o = final ? out + (long long)b * c + q * 4 : out + ((long long)b * gridDim.y + sp) * c + q * 4;
    *reinterpret_cast<float4*>(o) = acc;
  }
}

// partials [batch][splits][C] -> r [batch][C], the splits in sequence; one thread per (image, channel quad)
__global__ void __launch_bounds__(LA_NT) linattn_coldot_merge_kernel(const float* __restrict__ part,
                                                                     float* __restrict__ r, int batch, int c,
                                                                     int splits) {
  const int quads = c >> 2;
  const int e = blockIdx.x * LA_NT + threadIdx.x;
  if (e >= batch * quads) return;
  const int b = e / quads, q = e - b * quads;
  const float* p = part + (long long)b * splits * c + q * 4;
  float4 a = *reinterpret_cast<const float4*>(p);
  for (int z = 1; z < splits; ++z) {
    const float4 a2 = *reinterpret_cast<const float4*>(p + (long long)z * c);
    a = float4{a.x + a2.x, a.y + a2.y, a.z + a2.z, a.w + a2.w};
  }
  *reinterpret_cast<float4*>(r + (long long)b * c + q * 4) = a;
}

static bool la_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the shared shape / layout contract of the entry points; `what` names the caller in the message
static int la_check(const char* what, const void* k, long long ldk, long long sk, int batch, int n, int c) {
  if (!k || batch <= 0 || n <= 0 || c <= 0) {
    set_error("linattn %s: null pointer or empty shape (batch %d, n %d, c %d)", what, batch, n, c);
    return MVAE_EINVAL;
  }
  if (c % 4 != 0) {
    set_error("linattn %s: c = %d breaks the contract c %% 4 == 0 (16-byte channel slices)", what, c);
    return MVAE_EINVAL;
  }
  if (ldk < c || ldk % 4 != 0 || sk % 4 != 0 || sk < 0 || !la_al16(k)) {
    set_error("linattn %s: the k slice needs ld >= c, ld %% 4 == 0, stride %% 4 == 0 and 16-byte alignment", what);
    return MVAE_EINVAL;
  }
  if (batch > 65535) {
    set_error("linattn %s: batch %d exceeds 65535", what, batch);
    return MVAE_EINVAL;
  }
  return MVAE_OK;
}

static int la_row_blocks(const LaTile& t, int batch, int n) {
  const long long want = cdiv(LA_BLOCKS, (long long)t.cgroups * batch);
  return (int)std::max<long long>(1, std::min<long long>(want, cdiv(n, t.rows)));
}

}  // namespace mvae

using namespace mvae;

extern "C" {

size_t mvae_linattn_workspace_bytes(int batch, int n, int c) {
  if (batch <= 0 || n <= 0 || c <= 0) return 0;
  int per, splits;
  la_splits(batch, n, c, &per, &splits);
  // the statistics partials [batch][splits][2][c] (none when unsplit), or the backward's r [batch][c] followed by
  // its partials [batch][splits][c]
  return (size_t)batch * c * sizeof(float) * (size_t)(splits > 1 ? 2 * splits : 1);
}

int mvae_linattn_kstats(const float* k, long long ldk, long long stride_k, float* stats, int batch, int n, int c,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = la_check("kstats", k, ldk, stride_k, batch, n, c)) return rc;
  if (!stats || !la_al16(stats)) { set_error("linattn kstats: stats must be a 16-byte aligned pointer"); return MVAE_EINVAL; }
  const LaTile t = la_tile(c);
  int per, splits;
  la_splits(batch, n, c, &per, &splits);
  hipStream_t st = (hipStream_t)stream;
  if (splits == 1) {
    hipLaunchKernelGGL(linattn_kstats_kernel, dim3(t.cgroups, 1, batch), dim3(LA_NT), 0, st, k, ldk, stride_k, stats, n,
                       c, t.tc_log2, per, 1);
    return launch_status();
  }
  const size_t need = (size_t)batch * splits * 2 * c * sizeof(float);
  if (!workspace || !la_al16(workspace) || workspace_bytes < need) {
    set_error("linattn kstats: workspace of %zu bytes needed (mvae_linattn_workspace_bytes), got %zu", need,
              workspace ? workspace_bytes : (size_t)0);
    return MVAE_EWORKSPACE;
  }
  hipLaunchKernelGGL(linattn_kstats_kernel, dim3(t.cgroups, splits, batch), dim3(LA_NT), 0, st, k, ldk, stride_k,
                     (float*)workspace, n, c, t.tc_log2, per, 0);
  hipLaunchKernelGGL(linattn_kstats_merge_kernel, dim3(cdiv((long long)batch * (c >> 2), LA_NT)), dim3(LA_NT), 0, st,
                     (const float*)workspace, stats, batch, c, splits);
  return launch_status();
}

int mvae_linattn_ksoftmax(const float* k, long long ldk, long long stride_k, const float* stats, float* ksm, int batch,
                          int n, int c, void* stream) {
  if (int rc = la_check("ksoftmax", k, ldk, stride_k, batch, n, c)) return rc;
  if (!stats || !ksm || !la_al16(stats) || !la_al16(ksm)) {
    set_error("linattn ksoftmax: stats and ksm must be 16-byte aligned pointers");
    return MVAE_EINVAL;
  }
  const LaTile t = la_tile(c);
  hipLaunchKernelGGL(linattn_apply_kernel<0>, dim3(t.cgroups, la_row_blocks(t, batch, n), batch), dim3(LA_NT), 0,
                     (hipStream_t)stream, k, ldk, stride_k, stats, (const float*)nullptr, ksm, (long long)c,
                     (long long)n * c, n, c, t.tc_log2);
  return launch_status();
}

int mvae_linattn_dk(const float* k, long long ldk, long long stride_k, const float* stats, float* dk, long long lddk,
                    long long stride_dk, int batch, int n, int c, void* workspace, size_t workspace_bytes,
                    void* stream) {
  if (int rc = la_check("dk", k, ldk, stride_k, batch, n, c)) return rc;
  if (!stats || !dk || !la_al16(stats) || !la_al16(dk)) {
    set_error("linattn dk: stats and dk must be 16-byte aligned pointers");
    return MVAE_EINVAL;
  }
  if (lddk < c || lddk % 4 != 0 || stride_dk % 4 != 0 || stride_dk < 0) {
    set_error("linattn dk: the dk slice needs ld >= c, ld %% 4 == 0 and stride %% 4 == 0");
    return MVAE_EINVAL;
  }
  const LaTile t = la_tile(c);
  int per, splits;
  la_splits(batch, n, c, &per, &splits);
  const size_t rbytes = (size_t)batch * c * sizeof(float);
  const size_t need = rbytes * (size_t)(splits > 1 ? 1 + splits : 1);
  if (!workspace || !la_al16(workspace) || workspace_bytes < need) {
    set_error("linattn dk: workspace of %zu bytes needed (mvae_linattn_workspace_bytes), got %zu", need,
              workspace ? workspace_bytes : (size_t)0);
    return MVAE_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* r = (float*)workspace;
  if (splits == 1) {
    hipLaunchKernelGGL(linattn_coldot_kernel, dim3(t.cgroups, 1, batch), dim3(LA_NT), 0, st, k, ldk, stride_k, stats,
                       (const float*)dk, lddk, stride_dk, r, n, c, t.tc_log2, per, 1);
  } else {
    float* part = r + (size_t)batch * c;
    hipLaunchKernelGGL(linattn_coldot_kernel, dim3(t.cgroups, splits, batch), dim3(LA_NT), 0, st, k, ldk, stride_k,
                       stats, (const float*)dk, lddk, stride_dk, part, n, c, t.tc_log2, per, 0);
    hipLaunchKernelGGL(linattn_coldot_merge_kernel, dim3(cdiv((long long)batch * (c >> 2), LA_NT)), dim3(LA_NT), 0, st,
                       (const float*)part, r, batch, c, splits);
  }
  hipLaunchKernelGGL(linattn_apply_kernel<1>, dim3(t.cgroups, la_row_blocks(t, batch, n), batch), dim3(LA_NT), 0, st, k,
                     ldk, stride_k, stats, (const float*)r, dk, lddk, stride_dk, n, c, t.tc_log2);
  return launch_status();
}

}  // extern "C"
