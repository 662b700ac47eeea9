// Kernel distance (KID) on a similarity matrix (gfx950): the one reduction of contrad_amd/kid.py.
//
//   kid_sums    sum over a block of S of k(s) with the column self0 + row left out of every row by index; k is chosen
//               by the run-time `kind` (wave-uniform): 0, (gamma * s + coef0)^3; 1, the rational-quadratic mixture
//               sum over alpha in {1/2, 1, 2} of (1 + u / (2 alpha))^-alpha at u = max(2 - 2 s, 0), the squared distance
//               of two unit vectors (IEEE sqrt and division only).  Every term is formed and added in float64.  The row-tile
//               walk is csrc/simrow.h's (shared with prdc.hip), on 4 * rpw rows x 256 columns: rpw = 32, or 4 where
//               that would leave fewer than 1024 workgroups (a 1000 x 1000 block is 252 of them instead of 32).  A
//               lane sums its terms in row order, the wave by a butterfly, the four waves in wave order: one float64
//               partial per workgroup into the workspace.
//               kind 2 (contrad_dot_sums only) takes a second operand T of the same shape, with a leading dimension and a
//               vec_ok of its own, walked by the same load_tile behind the wave-uniform branch on `kind`: the term is
//               (double)s * (double)t, exact in float64, and nothing is left out.  Kinds 0 and 1 load no T tile.
//               kind 3 (contrad_gauss_sums only; contrad_amd/contrast.py's uniformity) is the Gaussian potential of two
//               unit vectors, exp(-t u) at u = max(2 - 2 s, 0), t in the `gamma` argument: one float64 multiply and one
//               float64 exp per term, in a loop of its own behind the same kind of wave-uniform branch.
//   kid_final   one workgroup adds the partials in a fixed order (thread t the partials t, t + 256, ...; then a tree
//               in LDS) and one thread adds the old value last when `accumulate` is set.
// No atomics: out[0] depends on no order of arrival, two calls are bitwise equal.
#include "../../include/contrad_hip.h"
#include "simrow.h"

#include <math.h>

namespace {

constexpr int KID_THREADS = simrow::THREADS;
constexpr int KID_COLS = simrow::COLS;
constexpr int KID_RPW_MAX = 32;                     // rows per wave of a tile
constexpr int KID_RPW_MIN = 4;
constexpr long long KID_ENOUGH_BLOCKS = 1024;
constexpr int KID_KIND_DOT = 2;                     // internal: the product of two operands (contrad_dot_sums)
constexpr int KID_KIND_GAUSS = 3;                   // internal: exp(-t u) (contrad_gauss_sums)

struct KidPlan {
  long long ctiles, blocks;
  int rpw;
};

// A function of (M, n) alone: the workspace query and the launcher agree, and so do two calls.
KidPlan kid_plan(int M, int n) {
  KidPlan p;
  p.ctiles = cdivll(n, KID_COLS);
  p.rpw = p.ctiles * cdivll(M, 4 * KID_RPW_MAX) >= KID_ENOUGH_BLOCKS ? KID_RPW_MAX : KID_RPW_MIN;
  p.blocks = p.ctiles * cdivll(M, 4 * p.rpw);
  return p;
}

// One term in float64.  kind 1: a NaN stays a NaN through the comparison, an s slightly above 1 gives u = 0.
__device__ __forceinline__ double kid_term(int kind, float s, double gamma, double coef0) {
  if (kind == 0) {
    const double x = gamma * (double)s + coef0;
    return x * x * x;
  }
  double u = 2.0 - 2.0 * (double)s;
  u = u < 0.0 ? 0.0 : u;
  const double q = 1.0 + 0.25 * u;
  return 1.0 / sqrt(1.0 + u) + 1.0 / (1.0 + 0.5 * u) + 1.0 / (q * q);
}

// Kind 2, a wave's rows of a tile: the same walk on both operands, a lane's products added in row order.
__device__ __forceinline__ double dot_rows(const float* __restrict__ S, long long ldS, const float* __restrict__ T, long long ldT,
                                           long long r0, int rows, long long c0, int n, int vec_ok, int vec_ok_t) {
  double acc = 0.0;
  for (int t0 = 0; t0 < rows; t0 += 4) {
    float v[4][4], t[4][4];
    simrow::load_tile(v, S, ldS, r0, t0, rows, c0, n, vec_ok, 0.f, [](int, long long) {});
    simrow::load_tile(t, T, ldT, r0, t0, rows, c0, n, vec_ok_t, 0.f, [](int, long long) {});
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool live = t0 + u < rows;                 // (uniform)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double k = (double)v[u][j] * (double)t[u][j];       // 24 x 24 bits: exact
        acc += live && c0 + j < n ? k : 0.0;
      }
    }
  }
  return acc;
}

// Kind 3, a wave's rows of a tile: the walk and the leave-out of kinds 0 and 1, the term exp(-t u) in float64.  A NaN stays a
// NaN through the comparison, an s slightly above 1 gives u = 0 and the term exp(-0) = 1.  exp in float64 needs more
// registers than the terms of kinds 0 and 1: with the 16 floats of a tile held beside it the kernel would pass from 70 to
// 78 VGPRs and from 7 to 6 waves per SIMD for every kind.  So a lane parks its tile in LDS (its own 16 words, column
// `tid`: no bank conflict, no barrier) and takes the cells back one at a time in a rolled loop, in the order u, j of the
// other kinds' loop.
__device__ __forceinline__ double gauss_rows(const float* __restrict__ S, long long ldS, long long r0, int rows, long long c0, int n,
                                             long long self0, double t, int vec_ok) {
  __shared__ float park[16][KID_THREADS];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int t0 = 0; t0 < rows; t0 += 4) {
    {
      float v[4][4];
      simrow::load_tile(v, S, ldS, r0, t0, rows, c0, n, vec_ok, 0.f, [](int, long long) {});
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) park[4 * u + j][tid] = v[u][j];
    }
#pragma unroll 1
    for (int q = 0; q < 16; ++q) {
      const int u = q >> 2, j = q & 3;
      const bool live = t0 + u < rows;                 // (uniform)
      const long long excl = self0 >= 0 ? self0 + r0 + 4 * (t0 + u) : -1;
      double d = 2.0 - 2.0 * (double)park[q][tid];     // exact: a float doubled and taken from 2 fits 53 bits
      d = d < 0.0 ? 0.0 : d;
      const double k = exp(-(t * d));
      const bool in = live && c0 + j < n && c0 + j != excl;       // left out by index: a select, so a NaN there is not seen
      acc += in ? k : 0.0;
    }
  }
  return acc;
}

// T may alias S (contrad_dot_sums with B = A): neither is written, so __restrict__ holds for both.
__global__ __launch_bounds__(KID_THREADS) void kid_sums_kernel(const float* __restrict__ S, long long ldS,
                                                               const float* __restrict__ T, long long ldT,
                                                               int M, int n, long long self0, int kind, double gamma,
                                                               double coef0, double* __restrict__ partial, int ctiles,
                                                               int rpw, int vec_ok, int vec_ok_t) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ct = blockIdx.x % ctiles, rt = blockIdx.x / ctiles;
  const long long c0 = (long long)ct * KID_COLS + 4 * lane;
  const long long r0 = (long long)rt * 4 * rpw + w;   // this wave's rows: r0, r0 + 4, ...
  int rows = r0 < M ? (int)min((long long)rpw, (M - r0 + 3) >> 2) : 0;

  double acc = 0.0;
  if (kind == KID_KIND_DOT) {                          // (uniform) the T tile stays out of the loop of kinds 0 and 1
    acc = dot_rows(S, ldS, T, ldT, r0, rows, c0, n, vec_ok, vec_ok_t);
    rows = 0;
  } else if (kind == KID_KIND_GAUSS) {                 // (uniform) and so does exp
    acc = gauss_rows(S, ldS, r0, rows, c0, n, self0, gamma, vec_ok);
    rows = 0;
  }
  for (int t0 = 0; t0 < rows; t0 += 4) {
    float v[4][4];
    simrow::load_tile(v, S, ldS, r0, t0, rows, c0, n, vec_ok, 0.f, [](int, long long) {});
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool live = t0 + u < rows;                 // (uniform)
      const long long excl = self0 >= 0 ? self0 + r0 + 4 * (t0 + u) : -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double k = kid_term(kind, v[u][j], gamma, coef0);
        const bool in = live && c0 + j < n && c0 + j != excl;     // left out by index: a select, so a NaN there is not seen
        acc += in ? k : 0.0;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) red[w] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(KID_THREADS) void kid_final_kernel(const double* __restrict__ partial, int nb, int accumulate,
                                                                double* __restrict__ out) {
  __shared__ double red[KID_THREADS];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int i = tid; i < nb; i += KID_THREADS) a += partial[i];
  red[tid] = a;
  __syncthreads();
  for (int s = KID_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[0] = accumulate ? out[0] + red[0] : red[0];   // the old value is added last
}

}  // namespace

extern "C" long long contrad_kid_sums_workspace_bytes(int M, int n) {
  if (M < 1 || n < 1) return -22;
  const KidPlan p = kid_plan(M, n);
  if (p.blocks > 0x7fffffffll) return -22;
  return p.blocks * (long long)sizeof(double);
}

namespace {

// T: the second operand of KID_KIND_DOT (null for the kinds of contrad_mmd_sums, which never read it).
int mmd_sums(const float* S, long long ldS, const float* T, long long ldT, int M, int n, long long self0, int kind, double gamma,
             double coef0, int accumulate, double* out, void* workspace, long long workspace_bytes, contrad_stream_t stream) {
  CONTRAD_ARG(S && out);
  CONTRAD_ARG(M >= 1 && n >= 1 && ldS >= n);
  CONTRAD_ARG(kind == 0 || kind == 1 || kind == KID_KIND_GAUSS || (kind == KID_KIND_DOT && T && ldT >= n));
  CONTRAD_ARG(isfinite(gamma) && isfinite(coef0));
  const KidPlan p = kid_plan(M, n);
  CONTRAD_ARG(p.blocks <= 0x7fffffffll);
  CONTRAD_ARG(workspace && workspace_bytes >= p.blocks * (long long)sizeof(double));
  CONTRAD_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0);
  const int vec_ok = (ldS % 4 == 0 && ((uintptr_t)S & 15) == 0) ? 1 : 0;
  const int vec_ok_t = (T && ldT % 4 == 0 && ((uintptr_t)T & 15) == 0) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(kid_sums_kernel, dim3((unsigned)p.blocks), dim3(KID_THREADS), 0, st, S, ldS, T, ldT, M, n, self0, kind,
                     gamma, coef0, partial, (int)p.ctiles, p.rpw, vec_ok, vec_ok_t);
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(kid_final_kernel, dim3(1), dim3(KID_THREADS), 0, st, partial, (int)p.blocks, accumulate ? 1 : 0, out);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int contrad_kid_sums(const float* S, long long ldS, int M, int n, long long self0, double gamma, double coef0,
                                int accumulate, double* out, void* workspace, long long workspace_bytes,
                                contrad_stream_t stream) {
  return mmd_sums(S, ldS, nullptr, 0, M, n, self0, 0, gamma, coef0, accumulate, out, workspace, workspace_bytes, stream);
}

extern "C" int contrad_mmd_sums(const float* S, long long ldS, int M, int n, long long self0, int kind, double gamma,
                                double coef0, int accumulate, double* out, void* workspace, long long workspace_bytes,
                                contrad_stream_t stream) {
  CONTRAD_ARG(kind == 0 || kind == 1);                 // the two-operand kind is contrad_dot_sums's alone
  return mmd_sums(S, ldS, nullptr, 0, M, n, self0, kind, gamma, coef0, accumulate, out, workspace, workspace_bytes, stream);
}

extern "C" int contrad_dot_sums(const float* A, long long ldA, const float* B, long long ldB, int M, int n, int accumulate,
                                double* out, void* workspace, long long workspace_bytes, contrad_stream_t stream) {
  CONTRAD_ARG(A && B);
  return mmd_sums(A, ldA, B, ldB, M, n, -1, KID_KIND_DOT, 1.0, 0.0, accumulate, out, workspace, workspace_bytes, stream);
}

extern "C" int contrad_gauss_sums(const float* S, long long ldS, int M, int n, long long self0, double t, int accumulate,
                                  double* out, void* workspace, long long workspace_bytes, contrad_stream_t stream) {
  CONTRAD_ARG(isfinite(t) && t >= 0.0);                // (a NaN compares false)
  return mmd_sums(S, ldS, nullptr, 0, M, n, self0, KID_KIND_GAUSS, t, 0.0, accumulate, out, workspace, workspace_bytes, stream);
}
