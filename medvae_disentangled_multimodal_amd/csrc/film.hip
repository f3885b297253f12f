// FiLM modulation of an NHWC feature map (src/models/conditional_vae.py FiLMLayer.forward: features * scale + shift with
// scale, shift [B][C] broadcast over the pixels), and its backward:
//   fwd        y[b][p][c] = x[b][p][c] * scale[b][c] + shift[b][c]
//   bwd        dx = dy * scale (optional), dscale[b][c] = sum_p dy * x, dshift[b][c] = sum_p dy -- x and dy read once
// Bandwidth-bound: the forward moves 2 B P C 4 bytes, the backward 3 B P C 4 (2 with dx skipped).
// A workgroup of 256 threads covers TC channel units (V = 4 channels per unit on the 16-byte path, 1 on the scalar
// path) x 256 / TC pixel rows and walks a fixed range of `ppw` pixels of one sample; its scale / shift come through LDS
// once. The backward's pixel sums are deterministic: every thread adds its pixels in index order, the rows of a
// workgroup are merged by a fixed tree in LDS, each workgroup writes one partial per channel to the workspace
//   ws = pscale [B][nchunk][C] | pshift [B][nchunk][C]          (fp32)
// and a second launch adds the nchunk partials of each (b, c) in index order. The pixel split depends on the shape
// alone (film_plan), so two runs -- eager, graph replay, any data-parallel replica -- add in the same order. No atomics.
#include "common.h"

#include <algorithm>

namespace mvae {

constexpr int FILM_NT = 256;
constexpr int FILM_MAXTC = 64;  // channel units per workgroup (256 channels on the 16-byte path)

struct FilmPlan {
  int tc_log2;     // channel units per workgroup = 1 << tc_log2 (threads of one pixel row)
  int cchunks;     // workgroups along the channels
  int ppw;         // pixels per workgroup
  int nchunk;      // workgroups along one sample's pixels
  size_t bytes;    // backward workspace
};

// iters = pixels per thread: 32 where the grid still fills the chip (1024 workgroups), halved down to 4 otherwise, so
// a small batch with many pixels (2 x C x 64 x 64) is shared by many workgroups per sample
static FilmPlan film_plan(int nb, int npix, int c, int v, int max_iters) {
  FilmPlan p;
  const int cu = c / v;
  p.tc_log2 = 0;
  while ((1 << p.tc_log2) < cu && (1 << p.tc_log2) < FILM_MAXTC) ++p.tc_log2;
  const int tc = 1 << p.tc_log2, rows = FILM_NT / tc;
  p.cchunks = cdiv(cu, tc);
  int iters = max_iters;
  while (iters > 4 && (long long)nb * p.cchunks * cdiv(npix, (long long)rows * iters) < 1024) iters >>= 1;
  p.ppw = rows * iters;
  p.nchunk = cdiv(npix, p.ppw);
  p.bytes = (size_t)2 * nb * p.nchunk * c * sizeof(float);
  return p;
}

template <int V>
struct FilmVec;
template <>
struct FilmVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ void get(const T& t, float* f) { f[0] = t.x, f[1] = t.y, f[2] = t.z, f[3] = t.w; }
  static __device__ __forceinline__ T put(const float* f) { return T{f[0], f[1], f[2], f[3]}; }
};
template <>
struct FilmVec<1> {
  typedef float T;
  static __device__ __forceinline__ void get(const T& t, float* f) { f[0] = t; }
  static __device__ __forceinline__ T put(const float* f) { return f[0]; }
};

// the workgroup's channel range of one [B][C] vector into LDS
__device__ __forceinline__ void film_stage(const float* __restrict__ src, float* dst, long long base, int n) {
  for (int i = threadIdx.x; i < n; i += FILM_NT) dst[i] = src[base + i];
}

// grid: (B * nchunk, cchunks)
template <int V>
__global__ void __launch_bounds__(FILM_NT) film_fwd_kernel(const float* __restrict__ x, long long ldx,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, float* __restrict__ y,
                                                           int npix, int c, int tc_log2, int ppw, int nchunk) {
  typedef typename FilmVec<V>::T T;
  __shared__ float ssc[FILM_MAXTC * V], ssh[FILM_MAXTC * V];
  const int tc = threadIdx.x & ((1 << tc_log2) - 1), row = threadIdx.x >> tc_log2, rows = FILM_NT >> tc_log2;
  const int b = blockIdx.x / nchunk, pc = blockIdx.x - b * nchunk;
  const int c0 = blockIdx.y * (V << tc_log2);
  const int nc = min(V << tc_log2, c - c0);
  film_stage(scale, ssc, (long long)b * c + c0, nc);
  film_stage(shift, ssh, (long long)b * c + c0, nc);
  __syncthreads();
  if (tc * V >= nc) return;
  float sc[V], sh[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sc[j] = ssc[tc * V + j], sh[j] = ssh[tc * V + j];
  const int pend = min(npix, (pc + 1) * ppw);
  const long long img = (long long)b * npix;
  const int ch = c0 + tc * V;
#pragma unroll 4
  for (int p = pc * ppw + row; p < pend; p += rows) {
    float xv[V], yv[V];
    FilmVec<V>::get(*reinterpret_cast<const T*>(x + (img + p) * ldx + ch), xv);
#pragma unroll
    for (int j = 0; j < V; ++j) yv[j] = fmaf(xv[j], sc[j], sh[j]);
    *reinterpret_cast<T*>(y + (img + p) * (long long)c + ch) = FilmVec<V>::put(yv);
  }
}

// grid: (B * nchunk, cchunks); pscale / pshift [B][nchunk][C]
template <int V>
__global__ void __launch_bounds__(FILM_NT) film_bwd_kernel(const float* __restrict__ x, long long ldx,
                                                           const float* __restrict__ dy, long long lddy,
                                                           const float* __restrict__ scale, float* __restrict__ dx,
                                                           float* __restrict__ pscale, float* __restrict__ pshift,
                                                           int npix, int c, int tc_log2, int ppw, int nchunk,
                                                           int write_dx) {
  typedef typename FilmVec<V>::T T;
  __shared__ float ssc[FILM_MAXTC * V];
  __shared__ float ra[FILM_NT * V], rb[FILM_NT * V];
  const int tc = threadIdx.x & ((1 << tc_log2) - 1), row = threadIdx.x >> tc_log2, rows = FILM_NT >> tc_log2;
  const int b = blockIdx.x / nchunk, pc = blockIdx.x - b * nchunk;
  const int c0 = blockIdx.y * (V << tc_log2);
  const int nc = min(V << tc_log2, c - c0);
  if (write_dx) film_stage(scale, ssc, (long long)b * c + c0, nc);
  __syncthreads();
  const bool live = tc * V < nc;
  float sc[V], as[V], ab[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sc[j] = (write_dx && live) ? ssc[tc * V + j] : 0.f, as[j] = ab[j] = 0.f;
  const int pend = min(npix, (pc + 1) * ppw);
  const long long img = (long long)b * npix;
  const int ch = c0 + tc * V;
  if (live) {
#pragma unroll 4
    for (int p = pc * ppw + row; p < pend; p += rows) {  // this thread's pixels, in index order
      float xv[V], gv[V], dv[V];
      FilmVec<V>::get(*reinterpret_cast<const T*>(x + (img + p) * ldx + ch), xv);
      FilmVec<V>::get(*reinterpret_cast<const T*>(dy + (img + p) * lddy + ch), gv);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        as[j] = fmaf(gv[j], xv[j], as[j]);
        ab[j] += gv[j];
        dv[j] = gv[j] * sc[j];
      }
      if (write_dx) *reinterpret_cast<T*>(dx + (img + p) * (long long)c + ch) = FilmVec<V>::put(dv);
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) ra[threadIdx.x * V + j] = as[j], rb[threadIdx.x * V + j] = ab[j];
  __syncthreads();
  for (int h = rows >> 1; h >= 1; h >>= 1) {  // fixed-order tree over the pixel rows
    if (row < h) {
      const int o = (threadIdx.x + (h << tc_log2)) * V;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        as[j] += ra[o + j], ab[j] += rb[o + j];
        ra[threadIdx.x * V + j] = as[j], rb[threadIdx.x * V + j] = ab[j];
      }
    }
    __syncthreads();
  }
  if (row == 0 && live) {
    const long long o = ((long long)b * nchunk + pc) * c + ch;
    *reinterpret_cast<T*>(pscale + o) = FilmVec<V>::put(as);
    *reinterpret_cast<T*>(pshift + o) = FilmVec<V>::put(ab);
  }
}

// one thread per (b, c): the nchunk partials in index order
__global__ void __launch_bounds__(FILM_NT) film_bwd_final_kernel(const float* __restrict__ pscale,
                                                                 const float* __restrict__ pshift, int nb, int c,
                                                                 int nchunk, float* __restrict__ dscale,
                                                                 float* __restrict__ dshift) {
  const long long e = (long long)blockIdx.x * FILM_NT + threadIdx.x;
  if (e >= (long long)nb * c) return;
  const long long b = e / c, ch = e - b * c;
  const long long o = b * nchunk * c + ch;
  float a = 0.f, s = 0.f;
  for (int k = 0; k < nchunk; ++k) a += pscale[o + (long long)k * c], s += pshift[o + (long long)k * c];
  dscale[e] = a;
  dshift[e] = s;
}

static bool film_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace mvae

using namespace mvae;

extern "C" {

// (the query does not know the alignment of the tensors: the larger of the two paths' needs)
size_t mvae_film_workspace_bytes(int nb, int npix, int c) {
  if (nb <= 0 || npix <= 0 || c <= 0) return 0;
  const size_t scalar = film_plan(nb, npix, c, 1, 32).bytes;
  return c % 4 == 0 ? std::max(scalar, film_plan(nb, npix, c, 4, 32).bytes) : scalar;
}

int mvae_film_fwd(const float* x, long long ldx, const float* scale, const float* shift, float* y, int nb, int npix,
                  int c, void* stream) {
  if (!x || !scale || !shift || !y || nb <= 0 || npix <= 0 || c <= 0 || ldx < c) {
    set_error("film_fwd: null pointer or bad shape (batch %d, pixels %d, channels %d, ld %lld)", nb, npix, c, ldx);
    return MVAE_EINVAL;
  }
  // 16-byte loads and stores only where every quad is aligned; any other layout takes the 4-byte path
  const bool vec = c % 4 == 0 && ldx % 4 == 0 && film_al16(x) && film_al16(y);
  const FilmPlan p = film_plan(nb, npix, c, vec ? 4 : 1, 8);
  if ((long long)nb * p.nchunk > 0x7FFFFFFFLL) {
    set_error("film_fwd: batch * pixel chunks exceeds the grid (%d x %d)", nb, p.nchunk);
    return MVAE_EINVAL;
  }
  const dim3 grid(nb * p.nchunk, p.cchunks);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(film_fwd_kernel<4>, grid, dim3(FILM_NT), 0, st, x, ldx, scale, shift, y, npix, c, p.tc_log2,
                       p.ppw, p.nchunk);
  else
    hipLaunchKernelGGL(film_fwd_kernel<1>, grid, dim3(FILM_NT), 0, st, x, ldx, scale, shift, y, npix, c, p.tc_log2,
                       p.ppw, p.nchunk);
  return launch_status();
}

int mvae_film_bwd(const float* x, long long ldx, const float* dy, long long lddy, const float* scale, float* dx,
                  float* dscale, float* dshift, int nb, int npix, int c, int write_dx, void* workspace,
                  size_t workspace_bytes, void* stream) {
  if (!x || !dy || !dscale || !dshift || (write_dx && (!dx || !scale)) || nb <= 0 || npix <= 0 || c <= 0 || ldx < c ||
      lddy < c) {
    set_error("film_bwd: null pointer or bad shape (batch %d, pixels %d, channels %d, ld %lld / %lld)", nb, npix, c,
              ldx, lddy);
    return MVAE_EINVAL;
  }
  const bool vec = c % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0 && film_al16(x) && film_al16(dy) &&
                   (!write_dx || film_al16(dx)) && film_al16(workspace);
  const FilmPlan p = film_plan(nb, npix, c, vec ? 4 : 1, 32);
  if ((long long)nb * p.nchunk > 0x7FFFFFFFLL) {
    set_error("film_bwd: batch * pixel chunks exceeds the grid (%d x %d)", nb, p.nchunk);
    return MVAE_EINVAL;
  }
  if (!workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < p.bytes) {
    set_error("film_bwd: workspace of %zu bytes needed (mvae_film_workspace_bytes), got %zu", p.bytes,
              workspace ? workspace_bytes : (size_t)0);
    return MVAE_EWORKSPACE;
  }
  float* pscale = (float*)workspace;
  float* pshift = pscale + (size_t)nb * p.nchunk * c;
  const dim3 grid(nb * p.nchunk, p.cchunks);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(film_bwd_kernel<4>, grid, dim3(FILM_NT), 0, st, x, ldx, dy, lddy, scale, dx, pscale, pshift,
                       npix, c, p.tc_log2, p.ppw, p.nchunk, write_dx);
  else
    hipLaunchKernelGGL(film_bwd_kernel<1>, grid, dim3(FILM_NT), 0, st, x, ldx, dy, lddy, scale, dx, pscale, pshift,
                       npix, c, p.tc_log2, p.ppw, p.nchunk, write_dx);
  hipLaunchKernelGGL(film_bwd_final_kernel, dim3(cdiv((long long)nb * c, FILM_NT)), dim3(FILM_NT), 0, st,
                     (const float*)pscale, (const float*)pshift, nb, c, p.nchunk, dscale, dshift);
  return launch_status();
}

}  // extern "C"
