// Augmentations, consistency term and (2N,1) GAN loss of the baseline training modes (std / aug / aug_both with the CR /
// bCR penalties and DiffAugment): the reference's augment/spatial.py:14-40 (HorizontalFlipRandomCrop), third_party/diffaug.py
// (DiffAugment, ~25 element-wise launches and two advanced-indexing gathers per call), penalty.py:45-58 and the GAN terms of
// training/gan/{std,aug,aug_both}.py.  NCHW fp32 in and out, per-sample parameters drawn on the host (include/contrad_hip.h).
// Every sum has a fixed order (no float atomics); the backward passes are gathers over pre-images.
#include "common.h"
#include "../../include/contrad_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// HorizontalFlipRandomCrop: nearest-neighbour grid_sample of the flip + integer-shift affine grid with reflection padding
// (align_corners=False) is the index map  out[i][j] = in[refl(i + ky)][refl(cflip(j) + kx)].
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int refl(int t, int n) { return t < 0 ? -t - 1 : (t >= n ? 2 * n - 1 - t : t); }
// the forward's form: a shift outside (-n, n) in a corrupt parameter row must not become an out-of-bounds read
__device__ __forceinline__ int refl_in(int t, int n) { return min(max(refl(t, n), 0), n - 1); }

struct HfrtArgs {
  const float* x;
  float* y;
  const float* params;
  int B, C, H, W;
};

// grid (B, parts); a thread makes 4 consecutive output columns of one row (VEC) or one pixel
template <bool VEC>
__global__ __launch_bounds__(256) void hfrt_fwd_kernel(HfrtArgs a) {
  const int n = blockIdx.x;
  const float* pr = a.params + (size_t)n * CONTRAD_HFRT_NPARAM;
  const bool flip = pr[0] < 0.f;
  const int kx = (int)pr[1], ky = (int)pr[2];
  const int H = a.H, W = a.W;
  const size_t base = (size_t)n * a.C * H * W;
  const float* src = a.x + base;
  float* dst = a.y + base;
  if (VEC) {
    const int W4 = W >> 2, total = a.C * H * W4;
    for (int q = blockIdx.y * blockDim.x + threadIdx.x; q < total; q += gridDim.y * blockDim.x) {
      const int row = q / W4, j0 = (q - row * W4) << 2;      // row = c * H + i
      const int c = row / H, i = row - c * H;
      const float* srow = src + ((size_t)c * H + refl_in(i + ky, H)) * W;
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + e;
        v[e] = srow[refl_in((flip ? W - 1 - j : j) + kx, W)];
      }
      *reinterpret_cast<f32x4*>(dst + (size_t)row * W + j0) = v;
    }
  } else {
    const int total = a.C * H * W;
    for (int q = blockIdx.y * blockDim.x + threadIdx.x; q < total; q += gridDim.y * blockDim.x) {
      const int row = q / W, j = q - row * W;
      const int c = row / H, i = row - c * H;
      dst[q] = src[((size_t)c * H + refl_in(i + ky, H)) * W + refl_in((flip ? W - 1 - j : j) + kx, W)];
    }
  }
}

// Pre-images of source index r under t -> refl(t + k) on [0, n): the direct one (t = r - k), the one reflected below 0 and
// the one reflected past n - 1, in this fixed order; every candidate is range-checked, so t[] needs three slots.  Returns
// their number.  Precondition |k| < n (the launcher checks max_pixels < W, the host draws |k| <= max_pixels): then the two
// reflected candidates exclude each other and there are at most two.  A corrupt parameter row outside it cannot read out of
// bounds here (unlike the forward, which clamps with refl_in); it would only sum the wrong outputs.
__device__ __forceinline__ int refl_preimages(int r, int k, int n, int* t) {
  int m = 0;
  const int d = r - k;
  if (d >= 0 && d < n) t[m++] = d;
  const int lo = -r - 1 - k;            // t + k = -r - 1 < 0
  if (lo >= 0 && lo < n) t[m++] = lo;
  const int hi = 2 * n - 1 - r - k;     // t + k = 2n - 1 - r >= n
  if (hi >= 0 && hi < n) t[m++] = hi;
  return m;
}

// adjoint: gin[r][q] = sum over the (at most 2 x 2) outputs that read (r, q), rows outer, columns inner
__global__ __launch_bounds__(256) void hfrt_bwd_kernel(HfrtArgs a) {   // x = grad_out, y = grad_in
  const int n = blockIdx.x;
  const float* pr = a.params + (size_t)n * CONTRAD_HFRT_NPARAM;
  const bool flip = pr[0] < 0.f;
  const int kx = (int)pr[1], ky = (int)pr[2];
  const int H = a.H, W = a.W;
  const size_t base = (size_t)n * a.C * H * W;
  const float* g = a.x + base;
  float* dst = a.y + base;
  const int total = a.C * H * W;
  for (int p = blockIdx.y * blockDim.x + threadIdx.x; p < total; p += gridDim.y * blockDim.x) {
    const int row = p / W, q = p - row * W;
    const int c = row / H, r = row - c * H;
    int ti[3], tj[3];
    const int ni = refl_preimages(r, ky, H, ti), nj = refl_preimages(q, kx, W, tj);
    float s = 0.f;
    for (int u = 0; u < ni; ++u) {
      const float* grow = g + ((size_t)c * H + ti[u]) * W;
      for (int v = 0; v < nj; ++v) s += grow[flip ? W - 1 - tj[v] : tj[v]];
    }
    dst[p] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// DiffAugment, policy bits 1 colour, 2 translation, 4 cutout (applied in this order).
// With u = 2x - 1 and per-sample b, s, c:  u1 = u + b,  u2 = (u1 - p) s + p (p = channel mean of u1 at the pixel),
// u3 = (u2 - M) c + M with M = mean(u2) = mean(u) + b (saturation keeps every pixel's channel mean): the per-sample mean of
// the input is the only reduction.  Translation reads (i + tx, j + ty), zero outside; cutout zeroes the clamped window.
// ------------------------------------------------------------------------------------------------------------------------
struct DaArgs {
  const float* x;       // forward: images; backward: grad_out
  float* y;             // forward: output; backward: grad_in
  const float* params;
  int B, H, W, policy;
};

struct DaSample {
  float b, s, c;
  int tx, ty;
  int r0, r1, c0, c1;   // cutout rows [r0, r1] x columns [c0, c1] (empty when r0 > r1)
};

__device__ __forceinline__ DaSample da_sample(const float* pr, int H, int W, int policy) {
  DaSample d;
  d.b = pr[0]; d.s = pr[1]; d.c = pr[2];
  d.tx = (policy & 2) ? (int)pr[3] : 0;
  d.ty = (policy & 2) ? (int)pr[4] : 0;
  d.r0 = 1; d.r1 = 0; d.c0 = 1; d.c1 = 0;
  if (policy & 4) {
    const int ch = (int)((float)H * 0.5f + 0.5f), cw = (int)((float)W * 0.5f + 0.5f);
    const int ox = (int)pr[5], oy = (int)pr[6];
    d.r0 = max(ox - ch / 2, 0); d.r1 = min(ox - ch / 2 + ch - 1, H - 1);
    d.c0 = max(oy - cw / 2, 0); d.c1 = min(oy - cw / 2 + cw - 1, W - 1);
    // (an offset so far out that the whole window clamps onto one border row / column: the reference zeroes that line)
    if (d.r1 < 0) d.r1 = 0;
    if (d.r0 > H - 1) d.r0 = H - 1;
    if (d.c1 < 0) d.c1 = 0;
    if (d.c0 > W - 1) d.c0 = W - 1;
  }
  return d;
}

__device__ __forceinline__ bool da_cut(const DaSample& d, int i, int j) {
  return i >= d.r0 && i <= d.r1 && j >= d.c0 && j <= d.c1;
}

// one output pixel (3 channels) from the source pixel values x0..x2 (already fetched at the translated position)
__device__ __forceinline__ void da_colour(float& u0, float& u1, float& u2, const DaSample& d, float M) {
  u0 += d.b; u1 += d.b; u2 += d.b;
  const float p = (u0 + u1 + u2) * (1.f / 3.f);
  u0 = (u0 - p) * d.s + p; u1 = (u1 - p) * d.s + p; u2 = (u2 - p) * d.s + p;
  u0 = (u0 - M) * d.c + M; u1 = (u1 - M) * d.c + M; u2 = (u2 - M) * d.c + M;
}

// forward of output pixels [p, p + NV) of image n; `src` = the image (LDS or global), NV consecutive columns of one row
template <int NV, typename SrcT>
__device__ __forceinline__ void da_fwd_pixels(const DaArgs& a, const DaSample& d, float M, SrcT src, float* dst, int p) {
  const int H = a.H, W = a.W, HW = H * W;
  const int i = p / W, j0 = p - i * W;
  float o[3][NV];
  const int si = i + d.tx;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    const int j = j0 + e, sj = j + d.ty;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (si >= 0 && si < H && sj >= 0 && sj < W && !da_cut(d, i, j)) {
      const int sp = si * W + sj;
      v0 = 2.f * src[sp] - 1.f; v1 = 2.f * src[HW + sp] - 1.f; v2 = 2.f * src[2 * HW + sp] - 1.f;
      if (a.policy & 1) da_colour(v0, v1, v2, d, M);
    }
    o[0][e] = 0.5f * v0 + 0.5f; o[1][e] = 0.5f * v1 + 0.5f; o[2][e] = 0.5f * v2 + 0.5f;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (NV == 4) {
      f32x4 v = {o[c][0], o[c][1], o[c][2], o[c][3]};
      *reinterpret_cast<f32x4*>(dst + c * HW + p) = v;
    } else {
      dst[c * HW + p] = o[c][0];
    }
  }
}

// sum of 3*HW floats of one image over the threads of a block slice [first, first + stride * k)
template <bool VEC>
__device__ __forceinline__ float da_partial_sum(const float* src, int n3, int first, int stride) {
  float s = 0.f;
  if (VEC) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
    for (int q = first; q < (n3 >> 2); q += stride) {
      const f32x4 v = s4[q];
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int q = first; q < n3; q += stride) s += src[q];
  }
  return s;
}

// ---- small images: one workgroup per image, the image staged in LDS ----
template <bool VEC>
__global__ __launch_bounds__(256) void diffaug_small_kernel(DaArgs a) {
  extern __shared__ __attribute__((aligned(16))) float img[];   // [3][H*W]
  __shared__ float red[16];
  const int n = blockIdx.x;
  const int HW = a.H * a.W, n3 = 3 * HW;
  const DaSample d = da_sample(a.params + (size_t)n * CONTRAD_DIFFAUG_NPARAM, a.H, a.W, a.policy);
  const float* src = a.x + (size_t)n * n3;
  float* dst = a.y + (size_t)n * n3;
  float s = 0.f;
  if (VEC) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
    f32x4* i4 = reinterpret_cast<f32x4*>(img);
    for (int q = threadIdx.x; q < (n3 >> 2); q += blockDim.x) {
      const f32x4 v = s4[q];
      i4[q] = v;
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int q = threadIdx.x; q < n3; q += blockDim.x) { const float v = src[q]; img[q] = v; s += v; }
  }
  s = block_sum(s, red);                                        // (its barriers also publish img)
  const float M = 2.f * (s / (float)n3) - 1.f + d.b;
  if (VEC) {
    for (int q = threadIdx.x; q < (HW >> 2); q += blockDim.x) da_fwd_pixels<4>(a, d, M, (const float*)img, dst, q << 2);
  } else {
    for (int p = threadIdx.x; p < HW; p += blockDim.x) da_fwd_pixels<1>(a, d, M, (const float*)img, dst, p);
  }
}

// ---- larger images: partial sums, then an apply pass ----
constexpr int DA_PART = 256 * 16;   // floats of 3*HW per partial block

template <bool VEC>
__global__ __launch_bounds__(256) void diffaug_sum_kernel(DaArgs a, float* __restrict__ partial) {   // partial[n][gridDim.y]
  __shared__ float red[16];
  const int n = blockIdx.x, n3 = 3 * a.H * a.W;
  const float* src = a.x + (size_t)n * n3;
  const int lo = blockIdx.y * DA_PART, hi = min(lo + DA_PART, n3);
  float s = 0.f;
  if (VEC) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
    for (int q = (lo >> 2) + threadIdx.x; q < (hi >> 2); q += blockDim.x) {
      const f32x4 v = s4[q];
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int q = lo + threadIdx.x; q < hi; q += blockDim.x) s += src[q];
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[(size_t)n * gridDim.y + blockIdx.y] = s;
}

__device__ __forceinline__ float da_total(const float* partial, int n, int nparts, float* sh) {
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int q = 0; q < nparts; ++q) s += partial[(size_t)n * nparts + q];
    *sh = s;
  }
  __syncthreads();
  return *sh;
}

template <bool VEC>
__global__ __launch_bounds__(256) void diffaug_apply_kernel(DaArgs a, const float* __restrict__ partial, int nparts) {
  __shared__ float tot;
  const int n = blockIdx.x;
  const int HW = a.H * a.W, n3 = 3 * HW;
  const DaSample d = da_sample(a.params + (size_t)n * CONTRAD_DIFFAUG_NPARAM, a.H, a.W, a.policy);
  const float M = 2.f * (da_total(partial, n, nparts, &tot) / (float)n3) - 1.f + d.b;
  const float* src = a.x + (size_t)n * n3;
  float* dst = a.y + (size_t)n * n3;
  if (VEC) {
    for (int q = blockIdx.y * blockDim.x + threadIdx.x; q < (HW >> 2); q += gridDim.y * blockDim.x)
      da_fwd_pixels<4>(a, d, M, src, dst, q << 2);
  } else {
    for (int p = blockIdx.y * blockDim.x + threadIdx.x; p < HW; p += gridDim.y * blockDim.x)
      da_fwd_pixels<1>(a, d, M, src, dst, p);
  }
}

// ---- backward.  g3[r][q] (at the colour stage's output) = 0.5 g[i][j] with (i, j) = (r - tx, q - ty) when that output
// pixel exists and is not cut, else 0;  gu2 = c g3 + (1 - c) mean_chw(g3);  gu1 = s gu2 + (1 - s) mean_c(gu2);  gx = 2 gu1.
// mean_chw(g3) sums the same terms wherever they sit, so it is taken over the OUTPUT pixels: one per-sample reduction. ----
__device__ __forceinline__ bool da_out_live(const DaArgs& a, const DaSample& d, int i, int j) {
  const int si = i + d.tx, sj = j + d.ty;           // the output pixel read an input pixel and was not cut
  return si >= 0 && si < a.H && sj >= 0 && sj < a.W && !da_cut(d, i, j);
}

// 0.5 * g masked, summed over output pixels [first, ...) of one image
__device__ __forceinline__ float da_bwd_partial(const DaArgs& a, const DaSample& d, const float* g, int lo, int hi,
                                                float* stage) {
  const int HW = a.H * a.W;
  float s = 0.f;
  for (int p = lo + threadIdx.x; p < hi; p += blockDim.x) {
    const int i = p / a.W, j = p - i * a.W;
    const bool live = da_out_live(a, d, i, j);
    const float g0 = live ? 0.5f * g[p] : 0.f, g1 = live ? 0.5f * g[HW + p] : 0.f, g2 = live ? 0.5f * g[2 * HW + p] : 0.f;
    if (stage) { stage[p] = g0; stage[HW + p] = g1; stage[2 * HW + p] = g2; }
    s += (g0 + g1) + g2;
  }
  return s;
}

// gradient of input pixels p .. p + NV - 1 (one row); G3(c, op) returns g3 of channel c at OUTPUT pixel op (live ones only)
template <int NV, bool STAGED>
__device__ __forceinline__ void da_bwd_pixels(const DaArgs& a, const DaSample& d, float mean3, const float* gsrc, float* dst,
                                              int p) {
  const int H = a.H, W = a.W, HW = H * W;
  const int r = p / W, q0 = p - r * W;
  const int i = r - d.tx;
  float o[3][NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    const int j = q0 + e - d.ty;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (i >= 0 && i < H && j >= 0 && j < W && !da_cut(d, i, j)) {
      const int op = i * W + j;
      if (STAGED) { g0 = gsrc[op]; g1 = gsrc[HW + op]; g2 = gsrc[2 * HW + op]; }
      else { g0 = 0.5f * gsrc[op]; g1 = 0.5f * gsrc[HW + op]; g2 = 0.5f * gsrc[2 * HW + op]; }
    }
    if (a.policy & 1) {
      const float k = (1.f - d.c) * mean3;
      g0 = d.c * g0 + k; g1 = d.c * g1 + k; g2 = d.c * g2 + k;
      const float m = (1.f - d.s) * ((g0 + g1 + g2) * (1.f / 3.f));
      g0 = d.s * g0 + m; g1 = d.s * g1 + m; g2 = d.s * g2 + m;
    }
    o[0][e] = 2.f * g0; o[1][e] = 2.f * g1; o[2][e] = 2.f * g2;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (NV == 4) {
      f32x4 v = {o[c][0], o[c][1], o[c][2], o[c][3]};
      *reinterpret_cast<f32x4*>(dst + c * HW + p) = v;
    } else {
      dst[c * HW + p] = o[c][0];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void diffaug_small_bwd_kernel(DaArgs a) {
  extern __shared__ __attribute__((aligned(16))) float img[];   // g3 at the output pixels, [3][H*W]
  __shared__ float red[16];
  const int n = blockIdx.x;
  const int HW = a.H * a.W, n3 = 3 * HW;
  const DaSample d = da_sample(a.params + (size_t)n * CONTRAD_DIFFAUG_NPARAM, a.H, a.W, a.policy);
  const float* g = a.x + (size_t)n * n3;
  float* dst = a.y + (size_t)n * n3;
  float s = da_bwd_partial(a, d, g, 0, HW, img);
  s = block_sum(s, red);
  const float mean3 = s / (float)n3;
  if (VEC) {
    for (int q = threadIdx.x; q < (HW >> 2); q += blockDim.x) da_bwd_pixels<4, true>(a, d, mean3, img, dst, q << 2);
  } else {
    for (int p = threadIdx.x; p < HW; p += blockDim.x) da_bwd_pixels<1, true>(a, d, mean3, img, dst, p);
  }
}

constexpr int DA_PIX_PART = 256 * 8;   // output pixels per partial block of the backward sum

__global__ __launch_bounds__(256) void diffaug_bwd_sum_kernel(DaArgs a, float* __restrict__ partial) {
  __shared__ float red[16];
  const int n = blockIdx.x, HW = a.H * a.W;
  const DaSample d = da_sample(a.params + (size_t)n * CONTRAD_DIFFAUG_NPARAM, a.H, a.W, a.policy);
  const int lo = blockIdx.y * DA_PIX_PART, hi = min(lo + DA_PIX_PART, HW);
  float s = da_bwd_partial(a, d, a.x + (size_t)n * 3 * HW, lo, hi, nullptr);
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[(size_t)n * gridDim.y + blockIdx.y] = s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void diffaug_bwd_apply_kernel(DaArgs a, const float* __restrict__ partial, int nparts) {
  __shared__ float tot;
  const int n = blockIdx.x;
  const int HW = a.H * a.W, n3 = 3 * HW;
  const DaSample d = da_sample(a.params + (size_t)n * CONTRAD_DIFFAUG_NPARAM, a.H, a.W, a.policy);
  const float mean3 = da_total(partial, n, nparts, &tot) / (float)n3;
  const float* g = a.x + (size_t)n * n3;
  float* dst = a.y + (size_t)n * n3;
  if (VEC) {
    for (int q = blockIdx.y * blockDim.x + threadIdx.x; q < (HW >> 2); q += gridDim.y * blockDim.x)
      da_bwd_pixels<4, false>(a, d, mean3, g, dst, q << 2);
  } else {
    for (int p = blockIdx.y * blockDim.x + threadIdx.x; p < HW; p += gridDim.y * blockDim.x)
      da_bwd_pixels<1, false>(a, d, mean3, g, dst, p);
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// Consistency term (penalty.py:45-58) and the GAN term of the (2N, 1) logit layout.  Single block, fixed order.
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(__expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + __expf(-x)); }

__global__ __launch_bounds__(256) void consistency_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b,
                                                          int ldb, int n0, int n1, float lbd0, float lbd1,
                                                          float* __restrict__ out, float* __restrict__ ga,
                                                          float* __restrict__ gb) {
  __shared__ float red[16];
  float s0 = 0.f, s1 = 0.f;
  const float w0 = n0 > 0 ? lbd0 / (float)n0 : 0.f, w1 = n1 > 0 ? lbd1 / (float)n1 : 0.f;
  for (int i = threadIdx.x; i < n0 + n1; i += blockDim.x) {
    const float d = a[(size_t)i * lda] - b[(size_t)i * ldb];
    const float w = i < n0 ? w0 : w1;
    if (i < n0) s0 += d * d; else s1 += d * d;
    const float g = 2.f * w * d;
    ga[i] = g;
    gb[i] = -g;
  }
  s0 = block_sum(s0, red);
  s1 = block_sum(s1, red);
  if (threadIdx.x == 0) out[0] = w0 * s0 + w1 * s1;
}

__global__ __launch_bounds__(256) void gan_d_loss_2n_kernel(const float* __restrict__ d, int ldd, int N, int kind,
                                                            float* __restrict__ out, float* __restrict__ grad) {
  __shared__ float red[16];
  float l = 0.f, sr = 0.f, sg = 0.f;
  const float invN = 1.f / (float)N;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const float r = d[(size_t)i * ldd], g = d[(size_t)(N + i) * ldd];
    float gr, gg;
    if (kind == 0) {          // nonsat: softplus(d_gen) + softplus(-d_real)
      l += softplus_f(g) + softplus_f(-r);
      gg = sigmoid_f(g); gr = -sigmoid_f(-r);
    } else if (kind == 1) {   // wgan
      l += g - r; gg = 1.f; gr = -1.f;
    } else if (kind == 2) {   // hinge
      l += fmaxf(1.f + g, 0.f) + fmaxf(1.f - r, 0.f);
      gg = (1.f + g > 0.f) ? 1.f : 0.f; gr = (1.f - r > 0.f) ? -1.f : 0.f;
    } else {                  // lsgan
      l += 0.5f * ((r - 1.f) * (r - 1.f) + g * g);
      gr = (r - 1.f); gg = g;
    }
    sr += r; sg += g;
    grad[i] = gr * invN;
    grad[N + i] = gg * invN;
  }
  l = block_sum(l, red);
  sr = block_sum(sr, red);
  sg = block_sum(sg, red);
  if (threadIdx.x == 0) { out[0] = l * invN; out[1] = sr * invN; out[2] = sg * invN; }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr long long DA_SMALL_BYTES = 16 * 1024;     // image (3 x H x W floats) staged in LDS up to here

inline int da_nparts(int H, int W) { return cdiv(3 * H * W, DA_PART); }
inline int da_bwd_nparts(int H, int W) { return cdiv(H * W, DA_PIX_PART); }

}  // namespace

extern "C" int contrad_hfrt(const float* x, float* y, const float* params, int B, int C, int H, int W, int max_pixels,
                            int adjoint, contrad_stream_t stream) {
  CONTRAD_ARG(x && y && params && x != y && B > 0 && C > 0 && H > 0 && W > 0 && H == W);
  CONTRAD_ARG(max_pixels >= 0 && max_pixels < W);
  CONTRAD_ARG((long long)C * H * W < (1ll << 31) && B <= 65535 * 32);
  HfrtArgs a{x, y, params, B, C, H, W};
  hipStream_t s = (hipStream_t)stream;
  const int work = C * H * W;
  if (adjoint) {
    hipLaunchKernelGGL(hfrt_bwd_kernel, dim3(B, min(cdiv(work, 256 * 4), 1024)), dim3(256), 0, s, a);
  } else if (W % 4 == 0 && aligned16(y)) {
    hipLaunchKernelGGL(hfrt_fwd_kernel<true>, dim3(B, min(cdiv(work / 4, 256 * 4), 1024)), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(hfrt_fwd_kernel<false>, dim3(B, min(cdiv(work, 256 * 4), 1024)), dim3(256), 0, s, a);
  }
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" long long contrad_diffaug_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)3 * H * W >= (1ll << 31)) return -22;
  if ((long long)3 * H * W * 4 <= DA_SMALL_BYTES) return 16;
  const int np = da_nparts(H, W) > da_bwd_nparts(H, W) ? da_nparts(H, W) : da_bwd_nparts(H, W);
  return (long long)B * np * (long long)sizeof(float);
}

extern "C" int contrad_diffaug(const float* x, float* y, const float* params, int B, int H, int W, int policy,
                               int backward, float* workspace, long long workspace_bytes, contrad_stream_t stream) {
  CONTRAD_ARG(x && y && params && x != y && B > 0 && H > 0 && W > 0 && policy > 0 && policy < 8);
  CONTRAD_ARG((long long)3 * H * W < (1ll << 31) && B <= 65535 * 32);
  DaArgs a{x, y, params, B, H, W, policy};
  hipStream_t s = (hipStream_t)stream;
  const bool vec = W % 4 == 0 && aligned16(x) && aligned16(y);
  const size_t img_bytes = (size_t)3 * H * W * sizeof(float);
  if ((long long)img_bytes <= DA_SMALL_BYTES) {
    if (backward) {
      if (vec) hipLaunchKernelGGL(diffaug_small_bwd_kernel<true>, dim3(B), dim3(256), img_bytes, s, a);
      else hipLaunchKernelGGL(diffaug_small_bwd_kernel<false>, dim3(B), dim3(256), img_bytes, s, a);
    } else {
      if (vec) hipLaunchKernelGGL(diffaug_small_kernel<true>, dim3(B), dim3(256), img_bytes, s, a);
      else hipLaunchKernelGGL(diffaug_small_kernel<false>, dim3(B), dim3(256), img_bytes, s, a);
    }
    CONTRAD_CHECK_LAUNCH();
    return 0;
  }
  CONTRAD_ARG(workspace && workspace_bytes >= contrad_diffaug_workspace_bytes(B, H, W));
  const int gy = min(cdiv(H * W, 256 * 4), 1024);
  if (backward) {
    const int np = da_bwd_nparts(H, W);
    hipLaunchKernelGGL(diffaug_bwd_sum_kernel, dim3(B, np), dim3(256), 0, s, a, workspace);
    CONTRAD_CHECK_LAUNCH();
    if (vec) hipLaunchKernelGGL(diffaug_bwd_apply_kernel<true>, dim3(B, gy), dim3(256), 0, s, a, workspace, np);
    else hipLaunchKernelGGL(diffaug_bwd_apply_kernel<false>, dim3(B, gy), dim3(256), 0, s, a, workspace, np);
  } else {
    const int np = da_nparts(H, W);
    if (vec) hipLaunchKernelGGL(diffaug_sum_kernel<true>, dim3(B, np), dim3(256), 0, s, a, workspace);
    else hipLaunchKernelGGL(diffaug_sum_kernel<false>, dim3(B, np), dim3(256), 0, s, a, workspace);
    CONTRAD_CHECK_LAUNCH();
    if (vec) hipLaunchKernelGGL(diffaug_apply_kernel<true>, dim3(B, gy), dim3(256), 0, s, a, workspace, np);
    else hipLaunchKernelGGL(diffaug_apply_kernel<false>, dim3(B, gy), dim3(256), 0, s, a, workspace, np);
  }
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_consistency(const float* a, int lda, const float* b, int ldb, int n0, int n1, float lbd0,
                                   float lbd1, float* out1, float* grad_a, float* grad_b, contrad_stream_t stream) {
  CONTRAD_ARG(a && b && out1 && grad_a && grad_b && n0 > 0 && n1 >= 0 && lda > 0 && ldb > 0);
  hipLaunchKernelGGL(consistency_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, n0, n1, lbd0, lbd1,
                     out1, grad_a, grad_b);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_gan_d_loss_2n(const float* logits, int ld, int N, int kind, float* out3, float* grad,
                                     contrad_stream_t stream) {
  CONTRAD_ARG(logits && out3 && grad && N > 0 && ld > 0 && kind >= 0 && kind <= 3);
  hipLaunchKernelGGL(gan_d_loss_2n_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, ld, N, kind, out3, grad);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
