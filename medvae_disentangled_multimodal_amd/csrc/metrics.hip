// On-device validation metrics (VAELightningModule.validation_step, src/lightning_module.py:220-300,
// via src/utils/metrics.py:14-73):
//   * SSIM as torchmetrics 1.7.4 structural_similarity_index_measure(preds, target, data_range):
//     11x11 Gaussian window (sigma 1.5), c1 = (0.01 R)^2, c2 = (0.03 R)^2, the map cropped by the
//     5-pixel reflect pad -- so only windows lying fully inside the image are evaluated and the
//     padding never contributes; per-image mean over (C, H-10, W-10).
//   * KL statistics of compute_kl_metrics on [B, z, h, w] (NHWC here): kl = 0.5(mu^2 + e^lv - lv - 1),
//     total, per-"sample" sums over dim 1 (the channel dim of a 4-D latent) -> their mean and
//     unbiased std, and the mean over all elements.
//   * Latent statistics of compute_latent_metrics (src/utils/metrics.py:76-101, the evaluation loop's per-batch call):
//     per-feature mean and unbiased std over the batch averaged over the features, and the |z| < 0.1 fraction.
// Reductions are fixed-order (double accumulation): results are reproducible run to run.
#include "common.h"
#include <algorithm>

namespace mvae {

constexpr int SSIM_K = 11, SSIM_PAD = 5;

// one workgroup per image; x, y NHWC [nb][h][w][c]
__global__ void __launch_bounds__(256) ssim_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                   int h, int w, int c, float c1, float c2,
                                                   float* __restrict__ per_image) {
  __shared__ float g[SSIM_K];
  __shared__ double part[256];
  if (threadIdx.x == 0) {  // torchmetrics _gaussian: exp(-(d/sigma)^2/2) normalised, d = -5..5 (fp32)
    float s = 0.f, t[SSIM_K];
    for (int i = 0; i < SSIM_K; ++i) {
      const float d = (float)(i - SSIM_PAD) / 1.5f;
      t[i] = expf(-(d * d) / 2.f);
      s += t[i];
    }
    for (int i = 0; i < SSIM_K; ++i) g[i] = t[i] / s;
  }
  __syncthreads();
  const int b = blockIdx.x;
  const int ho = h - 2 * SSIM_PAD, wo = w - 2 * SSIM_PAD;
  const long long img = (long long)b * h * w * c;
  const long long n = (long long)ho * wo * c;
  double acc = 0.0;
  for (long long e = threadIdx.x; e < n; e += blockDim.x) {
    const int ch = (int)(e % c);
    const long long q = e / c;
    const int j = (int)(q % wo) + SSIM_PAD, i = (int)(q / wo) + SSIM_PAD;
    float mx = 0.f, my = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
    for (int r = 0; r < SSIM_K; ++r) {
      const float* xr = x + img + ((long long)(i - SSIM_PAD + r) * w + (j - SSIM_PAD)) * c + ch;
      const float* yr = y + img + ((long long)(i - SSIM_PAD + r) * w + (j - SSIM_PAD)) * c + ch;
      for (int s = 0; s < SSIM_K; ++s) {
        const float wt = g[r] * g[s];
        const float a = xr[s * c], bb = yr[s * c];
        mx += wt * a;
        my += wt * bb;
        sxx += wt * a * a;
        syy += wt * bb * bb;
        sxy += wt * a * bb;
      }
    }
    const float vx = fmaxf(sxx - mx * mx, 0.f), vy = fmaxf(syy - my * my, 0.f);
    const float cxy = sxy - mx * my;
    const float v = ((2.f * mx * my + c1) * (2.f * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2));
    acc += (double)v;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) per_image[b] = (float)(part[0] / (double)n);
}

// per-pixel channel sums of the KL terms (mu/lv rows have stride ld >= zc)
__global__ void kl_pixel_sums_kernel(const float* __restrict__ mu, const float* __restrict__ lv, long long ld,
                                     long long npix, int zc, double* __restrict__ sums) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int k = 0; k < zc; ++k) {
      const float m = mu[p * ld + k], l = lv[p * ld + k];
      s += 0.5 * ((double)m * m + exp((double)l) - l - 1.0);
    }
    sums[p] = s;
  }
}

// out = {kl_total, kl_mean (over pixel sums), kl_std (unbiased), kl_per_dim_mean}
__global__ void __launch_bounds__(256) kl_stats_kernel(const double* __restrict__ sums, long long npix, int zc,
                                                       float* __restrict__ out) {
  __shared__ double part[256];
  double s = 0.0;
  for (long long p = threadIdx.x; p < npix; p += blockDim.x) s += sums[p];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  const double total = part[0];
  const double mean = total / (double)npix;
  __syncthreads();
  double v = 0.0;
  for (long long p = threadIdx.x; p < npix; p += blockDim.x) {
    const double d = sums[p] - mean;
    v += d * d;
  }
  part[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)total;
    out[1] = (float)mean;
    out[2] = npix > 1 ? (float)sqrt(part[0] / (double)(npix - 1)) : NAN;
    out[3] = (float)(total / ((double)npix * zc));
  }
}

// ---- latent statistics (compute_latent_metrics, src/utils/metrics.py:76-101) -------------------------------------
// z [batch][pixels][channels] (pixel stride ld >= channels, image stride sz), D = pixels * channels features:
//   latent_mean_avg = mean over the features of the per-feature mean over the batch,
//   latent_std_avg  = mean over the features of the per-feature unbiased std over the batch (NaN for batch = 1),
//   latent_sparsity = fraction of elements with |z| < 0.1 (strict; NaN is not sparse).
// All three are invariant under a permutation of the features, so the NHWC storage is read in place.
// A column reduction shaped like linattn_kstats_kernel: lanes run across features (16-B loads where base, ld, sz and
// channels allow, a 4-B path otherwise), the rows of the workgroup and a grid dimension run across the batch. Every
// thread keeps a Welford (count, mean, M2) triple per feature; triples are merged with Chan's parallel-variance
// formula in a fixed order -- the LDS tree over the workgroup's rows, then the batch splits in sequence -- without
// atomics: results are bitwise reproducible. The triples are accumulated and merged in DOUBLE, like the rest of this
// file: fp32 Welford keeps the mean on the fp32 grid, which for |mean| >> std (1000 +- 0.01) is as coarse as the
// deviations themselves. The sparsity count stays an integer until the final division.
constexpr int LS_NT = 256;           // threads per workgroup: tc feature lanes x (256 / tc) batch rows
constexpr int LS_BLOCKS = 512;       // workgroups the first pass aims for (two per CU)
constexpr int LS_MIN_ROWS = 32;      // samples per batch split at least
constexpr int LS_MAX_SPLITS = 1024;  // batch splits at most

struct LsPlan {
  int vec, tc_log2, cgroups, per, splits, merge_blocks;
  size_t off_counts, off_mean, off_m2, bytes;
};

// lanes across the feature units (quads or single features): the smallest power of two covering them, 64 at most;
// batch splits so that the launch reaches LS_BLOCKS workgroups while every split keeps LS_MIN_ROWS samples (c4's
// [256][8*8][256]: 64 feature groups x 8 splits = 512 workgroups). Workspace: per merge block a (sum of means, sum of
// stds) pair, per first-pass workgroup a sparsity count, then the partial means and M2s [splits][D].
static LsPlan ls_plan(int batch, long long d, int vec) {
  LsPlan p;
  p.vec = vec;
  const long long units = d / vec;
  int l = 0;
  while ((1LL << l) < units && l < 6) ++l;
  p.tc_log2 = l;
  p.cgroups = cdiv(units, 1 << l);
  const long long want = cdiv(LS_BLOCKS, p.cgroups);
  const long long cap = std::max(1, batch / LS_MIN_ROWS);
  const int s = (int)std::max<long long>(1, std::min<long long>(std::min(want, cap), LS_MAX_SPLITS));
  p.per = cdiv(batch, s);
  p.splits = cdiv(batch, p.per);
  p.merge_blocks = cdiv(d, LS_NT);
  p.off_counts = (size_t)p.merge_blocks * 2 * sizeof(double);
  p.off_mean = (p.off_counts + (size_t)p.cgroups * p.splits * sizeof(unsigned long long) + 15) & ~(size_t)15;
  p.off_m2 = p.off_mean + (size_t)p.splits * d * sizeof(double);
  p.bytes = p.off_m2 + (size_t)p.splits * d * sizeof(double);
  return p;
}

// (n, mean, m2) <- (n, mean, m2) merged with (nb, meanb, m2b); an empty side leaves the other unchanged
__device__ __forceinline__ void ls_merge(int n, double& mean, double& m2, int nb, double meanb, double m2b) {
  if (nb == 0) return;
  if (n == 0) {
    mean = meanb;
    m2 = m2b;
    return;
  }
  const double delta = meanb - mean, fb = (double)nb / (double)(n + nb);
  mean += delta * fb;
  m2 += m2b + delta * delta * ((double)n * fb);
}

// grid (feature groups, batch splits). V = 4: one channel quad per lane (16-B loads); V = 1: one feature per lane.
// pmean / pm2 [splits][d]: the split's mean and M2 per feature; counts [splits][feature groups]: |z| < 0.1 elements
template <int V>
__global__ void __launch_bounds__(LS_NT) latent_partial_kernel(const float* __restrict__ z, long long ld, long long sz,
                                                               int batch, int c, long long d, int tc_log2, int per,
                                                               double* __restrict__ pmean, double* __restrict__ pm2,
                                                               unsigned long long* __restrict__ counts) {
  __shared__ double sm[V][LS_NT], s2[V][LS_NT];
  __shared__ int sn[LS_NT];
  __shared__ unsigned long long sc[LS_NT];
  const int tid = threadIdx.x, tc = 1 << tc_log2, rows = LS_NT >> tc_log2;
  const int tx = tid & (tc - 1), ty = tid >> tc_log2;
  const long long e = ((long long)blockIdx.x * tc + tx) * V;  // first feature of this lane, in [pixel][channel] order
  const int sp = blockIdx.y;
  const int b0 = sp * per, b1 = min(batch, b0 + per);
  const bool live = e < d;
  int n = 0;
  unsigned cnt = 0;
  double mean[V], m2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) mean[j] = m2[j] = 0.0;
  if (live) {
    const long long pix = e / c;
    const float* p = z + pix * ld + (e - pix * c);
#pragma unroll 4
    for (int b = b0 + ty; b < b1; b += rows) {
      float x[V];
      if constexpr (V == 4) {
        const float4 v = *reinterpret_cast<const float4*>(p + (long long)b * sz);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
      } else {
        x[0] = p[(long long)b * sz];
      }
      const double inv = 1.0 / (double)++n;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double xv = (double)x[j], dl = xv - mean[j];
        mean[j] += dl * inv;
        m2[j] += dl * (xv - mean[j]);
        cnt += fabsf(x[j]) < 0.1f ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) sm[j][tid] = mean[j], s2[j][tid] = m2[j];
  sn[tid] = n;
  sc[tid] = cnt;
  __syncthreads();
  for (int h = rows >> 1; h >= 1; h >>= 1) {  // fixed-order tree over the batch rows
    if (ty < h) {
      const int o = tid + (h << tc_log2), nb = sn[o];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        ls_merge(n, mean[j], m2[j], nb, sm[j][o], s2[j][o]);
        sm[j][tid] = mean[j], s2[j][tid] = m2[j];
      }
      n += nb;
      sn[tid] = n;
    }
    __syncthreads();
  }
  if (ty == 0 && live) {
    double* om = pmean + (long long)sp * d + e;
    double* o2 = pm2 + (long long)sp * d + e;
#pragma unroll
    for (int j = 0; j < V; ++j) om[j] = mean[j], o2[j] = m2[j];
  }
  for (int o = LS_NT >> 1; o > 0; o >>= 1) {  // the workgroup's sparsity count
    if (tid < o) sc[tid] += sc[tid + o];
    __syncthreads();
  }
  if (tid == 0) counts[(long long)sp * gridDim.x + blockIdx.x] = sc[0];
}

// one thread per feature: the batch splits merged in sequence, std = sqrt(M2 / (batch - 1)); pairs [blocks][2] = the
// workgroup's (sum of means, sum of stds)
__global__ void __launch_bounds__(LS_NT) latent_merge_kernel(const double* __restrict__ pmean,
                                                             const double* __restrict__ pm2, long long d, int batch,
                                                             int per, int splits, double* __restrict__ pairs) {
  __shared__ double sa[LS_NT], sb[LS_NT];
  const long long f = (long long)blockIdx.x * LS_NT + threadIdx.x;
  double mean = 0.0, sd = 0.0;
  if (f < d) {
    int n = min(per, batch);
    mean = pmean[f];
    double m2 = pm2[f];
    for (int s = 1; s < splits; ++s) {
      const int nb = min(batch, (s + 1) * per) - s * per;
      ls_merge(n, mean, m2, nb, pmean[(long long)s * d + f], pm2[(long long)s * d + f]);
      n += nb;
    }
    sd = batch > 1 ? sqrt(m2 / (double)(batch - 1)) : (double)NAN;
  }
  sa[threadIdx.x] = mean;
  sb[threadIdx.x] = sd;
  __syncthreads();
  for (int o = LS_NT >> 1; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sa[threadIdx.x] += sa[threadIdx.x + o];
      sb[threadIdx.x] += sb[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) pairs[2 * blockIdx.x] = sa[0], pairs[2 * blockIdx.x + 1] = sb[0];
}

// out = {latent_mean_avg, latent_std_avg, latent_sparsity}
__global__ void __launch_bounds__(LS_NT) latent_final_kernel(const double* __restrict__ pairs, int nblocks,
                                                             const unsigned long long* __restrict__ counts,
                                                             int ncounts, long long d, int batch,
                                                             float* __restrict__ out) {
  __shared__ double sa[LS_NT], sb[LS_NT];
  __shared__ unsigned long long sc[LS_NT];
  double a = 0.0, b = 0.0;
  unsigned long long k = 0;
  for (int i = threadIdx.x; i < nblocks; i += LS_NT) a += pairs[2 * i], b += pairs[2 * i + 1];
  for (int i = threadIdx.x; i < ncounts; i += LS_NT) k += counts[i];
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b;
  sc[threadIdx.x] = k;
  __syncthreads();
  for (int o = LS_NT >> 1; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sa[threadIdx.x] += sa[threadIdx.x + o];
      sb[threadIdx.x] += sb[threadIdx.x + o];
      sc[threadIdx.x] += sc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(sa[0] / (double)d);
    out[1] = (float)(sb[0] / (double)d);
    out[2] = (float)((double)sc[0] / ((double)batch * (double)d));
  }
}

}  // namespace mvae

using namespace mvae;

extern "C" {

int mvae_ssim(const float* x, const float* y, int nb, int h, int w, int c, float data_range, float* per_image,
              void* stream) {
  if (nb <= 0 || c <= 0 || h < SSIM_K || w < SSIM_K) { set_error("ssim: images must be >= 11x11"); return MVAE_EINVAL; }
  const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
  hipLaunchKernelGGL(ssim_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, y, h, w, c, c1, c2, per_image);
  return launch_status();
}

size_t mvae_kl_stats_workspace_bytes(long long npix) { return (size_t)std::max<long long>(npix, 1) * sizeof(double); }

int mvae_kl_stats(const float* mu, const float* logvar, long long ld, long long npix, int zc, float* out,
                  void* workspace, size_t workspace_bytes, void* stream) {
  if (npix <= 0 || zc <= 0 || ld < zc) { set_error("kl_stats: bad sizes"); return MVAE_EINVAL; }
  if (workspace_bytes < (size_t)npix * sizeof(double)) { set_error("kl_stats: workspace"); return MVAE_EWORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)std::min<long long>((npix + 255) / 256, 4096);
  hipLaunchKernelGGL(kl_pixel_sums_kernel, dim3(blocks), dim3(256), 0, st, mu, logvar, ld, npix, zc, (double*)workspace);
  hipLaunchKernelGGL(kl_stats_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, npix, zc, out);
  return launch_status();
}

// (the query does not know the alignment of the tensor: the larger of the two paths' needs)
size_t mvae_latent_stats_workspace_bytes(int batch, int pixels, int channels) {
  if (batch <= 0 || pixels <= 0 || channels <= 0) return 0;
  const long long d = (long long)pixels * channels;
  const size_t scalar = ls_plan(batch, d, 1).bytes;
  return channels % 4 == 0 ? std::max(scalar, ls_plan(batch, d, 4).bytes) : scalar;
}

int mvae_latent_stats(const float* z, long long ld, long long stride_image, int batch, int pixels, int channels,
                      float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!z || !out || batch <= 0 || pixels <= 0 || channels <= 0) {
    set_error("latent_stats: null pointer or empty shape (batch %d, pixels %d, channels %d)", batch, pixels, channels);
    return MVAE_EINVAL;
  }
  const long long d = (long long)pixels * channels;
  if (ld < channels || stride_image < 0 || batch > (1 << 30) || d > (1LL << 31) - 1) {
    set_error("latent_stats: needs ld >= channels, stride_image >= 0, batch <= 2^30 and pixels * channels < 2^31");
    return MVAE_EINVAL;
  }
  // 16-byte loads only where every quad is aligned; any other layout takes the 4-byte path
  const bool vec = channels % 4 == 0 && ld % 4 == 0 && stride_image % 4 == 0 && ((uintptr_t)z & 15) == 0;
  const LsPlan p = ls_plan(batch, d, vec ? 4 : 1);
  if (!workspace || ((uintptr_t)workspace & 15) != 0 || workspace_bytes < p.bytes) {
    set_error("latent_stats: 16-byte aligned workspace of %zu bytes needed (mvae_latent_stats_workspace_bytes), got %zu",
              p.bytes, workspace ? workspace_bytes : (size_t)0);
    return MVAE_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* pairs = (double*)ws;
  unsigned long long* counts = (unsigned long long*)(ws + p.off_counts);
  double* pmean = (double*)(ws + p.off_mean);
  double* pm2 = (double*)(ws + p.off_m2);
  if (vec)
    hipLaunchKernelGGL(latent_partial_kernel<4>, dim3(p.cgroups, p.splits), dim3(LS_NT), 0, st, z, ld, stride_image,
                       batch, channels, d, p.tc_log2, p.per, pmean, pm2, counts);
  else
    hipLaunchKernelGGL(latent_partial_kernel<1>, dim3(p.cgroups, p.splits), dim3(LS_NT), 0, st, z, ld, stride_image,
                       batch, channels, d, p.tc_log2, p.per, pmean, pm2, counts);
  hipLaunchKernelGGL(latent_merge_kernel, dim3(p.merge_blocks), dim3(LS_NT), 0, st, (const double*)pmean,
                     (const double*)pm2, d, batch, p.per, p.splits, pairs);
  hipLaunchKernelGGL(latent_final_kernel, dim3(1), dim3(LS_NT), 0, st, (const double*)pairs, p.merge_blocks,
                     (const unsigned long long*)counts, p.cgroups * p.splits, d, batch, out);
  return launch_status();
}

}  // extern "C"
