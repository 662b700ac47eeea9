// Device side of the gradient penalty (--penalty=gp, the reference's penalty.py:16-42; WGAN-GP): the interpolation between
// the real and the generated batch, and  lbd * mean_n (||grad_n||_2 - 1)^2  with its gradient w.r.t. grad in the same pass.
// NCHW fp32, rows of L = C*H*W floats.  Every sum has a fixed order (no float atomics): two calls on the same inputs give
// bitwise equal outputs.
//
// Access: 16-byte loads / stores wherever the ADDRESS is 16-byte aligned.  A row of L % 4 != 0 floats starts at any of the
// four offsets, so a range is split into a scalar head up to the next aligned address, a vector body and a scalar tail
// (gp_split); with a base pointer that is not 16-byte aligned everything is scalar.
#include "common.h"
#include "../../include/contrad_hip.h"

namespace {

constexpr int GP_PART = 256 * 16;                   // floats of a row per block of the multi-block launches
constexpr long long GP_SMALL_BYTES = 16 * 1024;     // rows up to here: one workgroup per row, the row staged in LDS

struct GpSplit { int head, nvec, tail0; };          // scalar [0, head), vectors at head + 4k (k < nvec), scalar [tail0, cnt)

// split of `cnt` floats whose first one sits `abs0` floats behind a 16-byte aligned base
__device__ __forceinline__ GpSplit gp_split(long long abs0, int cnt, bool vec) {
  GpSplit r;
  if (!vec) { r.head = cnt; r.nvec = 0; r.tail0 = cnt; return r; }
  r.head = min(cnt, (int)((4 - (abs0 & 3)) & 3));
  r.nvec = (cnt - r.head) >> 2;
  r.tail0 = r.head + 4 * r.nvec;
  return r;
}

// alpha x + (1 - alpha) g as the reference writes it, each product and the sum rounded on its own (no contraction into an
// fma): with alpha == 1 the second factor is exactly 0 and 1 * x + 0 * g is x, with alpha == 0 it is 0 * x + 1 * g = g --
// the form  g + alpha (x - g)  would round x - g first and return g + (x - g) != x.  The two selects make the same hold for
// the bit pattern as well (x = -0 plus a product +0 would give +0) and for non-finite pixels (0 * inf).
__device__ __forceinline__ float gp_mix(float a, float b, float x, float g) {
  const float v = __fadd_rn(__fmul_rn(a, x), __fmul_rn(b, g));
  return a == 1.f ? x : (a == 0.f ? g : v);
}

// grid (N, parts): block (n, p) makes the ranges [lo, lo + GP_PART) of row n for lo = p * GP_PART, (p + parts) * GP_PART, ...
__global__ __launch_bounds__(256) void gp_interpolate_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ alpha, float* __restrict__ y, int L,
                                                             bool vec) {
  const int n = blockIdx.x;
  const float a = alpha[n], b = 1.f - a;
  const long long row = (long long)n * L;
  for (long long lo = (long long)blockIdx.y * GP_PART; lo < L; lo += (long long)gridDim.y * GP_PART) {
    const int cnt = (int)min((long long)GP_PART, L - lo);
    const float* xs = x + row + lo;
    const float* gs = g + row + lo;
    float* ys = y + row + lo;
    const GpSplit sp = gp_split(row + lo, cnt, vec);
    for (int q = threadIdx.x; q < sp.head; q += blockDim.x) ys[q] = gp_mix(a, b, xs[q], gs[q]);
    for (int k = threadIdx.x; k < sp.nvec; k += blockDim.x) {
      const int q = sp.head + 4 * k;
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + q), gv = *reinterpret_cast<const f32x4*>(gs + q);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = gp_mix(a, b, xv[e], gv[e]);
      *reinterpret_cast<f32x4*>(ys + q) = o;
    }
    for (int q = sp.tail0 + threadIdx.x; q < cnt; q += blockDim.x) ys[q] = gp_mix(a, b, xs[q], gs[q]);
  }
}

// d/d grad_n of lbd * mean_n (norm_n - 1)^2 is this factor times grad_n; 0 for a zero row (torch's 2-norm backward there).
// Only norm == 0 is special: a NaN / Inf norm gives a NaN factor, so a non-finite gradient reaches the parameter gradients as
// it does in torch instead of being masked.
__device__ __forceinline__ float gp_cot_scale(float norm, float lbd, int N) {
  return norm == 0.f ? 0.f : (2.f * lbd * (norm - 1.f)) / ((float)N * norm);
}

// sum of squares of `cnt` floats at src (thread-strided, fixed order); STAGE: also copied to lds[q + shift]
template <bool STAGE>
__device__ __forceinline__ float gp_sumsq(const float* src, const GpSplit& sp, int cnt, float* lds, int shift) {
  float s = 0.f;
  for (int q = threadIdx.x; q < sp.head; q += blockDim.x) {
    const float v = src[q];
    if (STAGE) lds[q + shift] = v;
    s += v * v;
  }
  for (int k = threadIdx.x; k < sp.nvec; k += blockDim.x) {
    const int q = sp.head + 4 * k;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + q);
    if (STAGE) *reinterpret_cast<f32x4*>(lds + q + shift) = v;       // (head + shift) % 4 == 0 whenever nvec > 0
    s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  for (int q = sp.tail0 + threadIdx.x; q < cnt; q += blockDim.x) {
    const float v = src[q];
    if (STAGE) lds[q + shift] = v;
    s += v * v;
  }
  return s;
}

// dst[q] = sc * src[q + shift] over the same split (src: the LDS copy with its shift, or the row itself with shift 0)
__device__ __forceinline__ void gp_scale_out(const float* src, int shift, float* dst, const GpSplit& sp, int cnt, float sc) {
  for (int q = threadIdx.x; q < sp.head; q += blockDim.x) dst[q] = sc * src[q + shift];
  for (int k = threadIdx.x; k < sp.nvec; k += blockDim.x) {
    const int q = sp.head + 4 * k;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + q + shift);
    const f32x4 o = {sc * v[0], sc * v[1], sc * v[2], sc * v[3]};
    *reinterpret_cast<f32x4*>(dst + q) = o;
  }
  for (int q = sp.tail0 + threadIdx.x; q < cnt; q += blockDim.x) dst[q] = sc * src[q + shift];
}

// ---- small rows: one workgroup per row, staged in LDS while it is summed, scaled out of LDS ----
__global__ __launch_bounds__(256) void gp_penalty_small_kernel(const float* __restrict__ grad, float* __restrict__ norms,
                                                               float* __restrict__ cot, int N, int L, float lbd, bool vec) {
  extern __shared__ __attribute__((aligned(16))) float row_lds[];     // L + 4 floats: the row at offset `shift`
  __shared__ float red[16];
  const int n = blockIdx.x;
  const long long row = (long long)n * L;
  const GpSplit sp = gp_split(row, L, vec);
  const int shift = vec ? (int)(row & 3) : 0;       // keeps the vector body 16-byte aligned in LDS as it is in memory
  float s = gp_sumsq<true>(grad + row, sp, L, row_lds, shift);
  s = block_sum(s, red);                            // (its barriers also publish row_lds)
  const float norm = sqrtf(s);
  if (threadIdx.x == 0) norms[n] = norm;
  gp_scale_out(row_lds, shift, cot + row, sp, L, gp_cot_scale(norm, lbd, N));
}

// ---- larger rows: partial sums of GP_PART floats, then an apply pass over the same parts ----
__global__ __launch_bounds__(256) void gp_penalty_sum_kernel(const float* __restrict__ grad, float* __restrict__ partial,
                                                             int L, bool vec) {              // partial[n][gridDim.y]
  __shared__ float red[16];
  const int n = blockIdx.x;
  const long long row = (long long)n * L;
  const int lo = blockIdx.y * GP_PART, cnt = min(GP_PART, L - lo);
  const GpSplit sp = gp_split(row + lo, cnt, vec);
  float s = gp_sumsq<false>(grad + row + lo, sp, cnt, nullptr, 0);
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[(size_t)n * gridDim.y + blockIdx.y] = s;
}

__global__ __launch_bounds__(256) void gp_penalty_apply_kernel(const float* __restrict__ grad,
                                                               const float* __restrict__ partial, float* __restrict__ norms,
                                                               float* __restrict__ cot, int N, int L, float lbd, bool vec) {
  __shared__ float tot;
  const int n = blockIdx.x;
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int q = 0; q < (int)gridDim.y; ++q) s += partial[(size_t)n * gridDim.y + q];
    tot = s;
  }
  __syncthreads();
  const float norm = sqrtf(tot);
  if (blockIdx.y == 0 && threadIdx.x == 0) norms[n] = norm;
  const long long row = (long long)n * L;
  const int lo = blockIdx.y * GP_PART, cnt = min(GP_PART, L - lo);
  const GpSplit sp = gp_split(row + lo, cnt, vec);
  gp_scale_out(grad + row + lo, 0, cot + row + lo, sp, cnt, gp_cot_scale(norm, lbd, N));
}

// ---- the scalar: out[0] = lbd / N * sum_n (norm_n - 1)^2, one block, fixed order ----
__global__ __launch_bounds__(256) void gp_penalty_value_kernel(const float* __restrict__ norms, float* __restrict__ out, int N,
                                                               float lbd) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const float d = norms[i] - 1.f;
    s += d * d;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = lbd * (s / (float)N);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool gp_small(long long L) { return L * (long long)sizeof(float) <= GP_SMALL_BYTES; }
inline bool gp_size_ok(int N, long long L) {                  // rows index with int, grid.y of the two-launch form
  return N > 0 && L > 0 && L < (1ll << 31) && cdivll(L, GP_PART) <= 65535;
}

}  // namespace

extern "C" int contrad_gp_interpolate(const float* x, const float* g, const float* alpha, float* xhat, int N, long long chw,
                                      contrad_stream_t stream) {
  CONTRAD_ARG(x && g && alpha && xhat && xhat != x && xhat != g);
  CONTRAD_ARG(gp_size_ok(N, chw));
  const bool vec = aligned16(x) && aligned16(g) && aligned16(xhat);
  const int parts = (int)(cdivll(chw, GP_PART) < 1024 ? cdivll(chw, GP_PART) : 1024);
  hipLaunchKernelGGL(gp_interpolate_kernel, dim3(N, parts), dim3(256), 0, (hipStream_t)stream, x, g, alpha, xhat, (int)chw,
                     vec);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" long long contrad_gp_penalty_workspace_bytes(int N, long long chw) {
  if (!gp_size_ok(N, chw)) return -22;
  if (gp_small(chw)) return 16;
  return (long long)N * cdivll(chw, GP_PART) * (long long)sizeof(float);
}

extern "C" int contrad_gp_penalty(const float* grad, float* norms, float* out1, float* cot, int N, long long chw, float lbd,
                                  float* workspace, long long workspace_bytes, contrad_stream_t stream) {
  CONTRAD_ARG(grad && norms && out1 && cot && cot != grad);
  CONTRAD_ARG(gp_size_ok(N, chw));
  hipStream_t s = (hipStream_t)stream;
  const bool vec = aligned16(grad) && aligned16(cot);
  const int L = (int)chw;
  if (gp_small(chw)) {
    hipLaunchKernelGGL(gp_penalty_small_kernel, dim3(N), dim3(256), (size_t)(L + 4) * sizeof(float), s, grad, norms, cot, N, L,
                       lbd, vec);
  } else {
    CONTRAD_ARG(workspace && workspace_bytes >= contrad_gp_penalty_workspace_bytes(N, chw));
    const int np = cdiv(L, GP_PART);
    hipLaunchKernelGGL(gp_penalty_sum_kernel, dim3(N, np), dim3(256), 0, s, grad, workspace, L, vec);
    CONTRAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(gp_penalty_apply_kernel, dim3(N, np), dim3(256), 0, s, grad, workspace, norms, cot, N, L, lbd, vec);
  }
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(gp_penalty_value_kernel, dim3(1), dim3(256), 0, s, norms, out1, N, lbd);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
