// Sliced Wasserstein distance on Laplacian-pyramid patches (gfx950): the device side of contrad_amd/swd.py.
//
//   swd_u8_planes     uint8 NHWC [n][R][R][3] -> fp32 planes [n * 3][R][R], the values 0 ... 255 as they are (exact).
//   swd_pyr_down      one Gaussian step: the 5 x 5 stencil outer(g, g), g = [1 4 6 4 1] / 16, at the even coordinates only; the
//                     mirror boundary (d c b | a b c d | c b a) is an index map, no padded copy.  25 products per output, the
//                     weights g_i g_j / 256 exact in fp32, added in the fixed order dy, dx.
//   swd_pyr_up_sub    fine -= up(coarse) in place.  up() convolves the zero-inserted coarse level (coarse at the even
//                     coordinates) with 4 outer(g, g) under the same mirror rule; the zero-insert is never made: a tap whose
//                     mirrored coordinate is odd is skipped, so a pixel reads at most 3 x 3 coarse samples (at an edge one
//                     sample through two taps: two products, as in the definition).
//   swd_gather        7 x 7 x 3 patches around given centres into the transposed bank [148][n_pad] (row c * 49 + dy * 7 + dx,
//                     row 147 and the columns [n_desc, n_pad) zero: features.py's packed layout), one thread per column, and
//                     per channel the float64 sum and sum of squares: a thread adds its 49 values per channel in row order,
//                     the wave by a butterfly, the waves in wave order, one partial per workgroup; swd_final adds the partials
//                     in a fixed order.  A centre outside [3, R - 4] is clamped into it: nothing outside the level is read.
//   swd_sort_tile /   rows of n floats ascending, in place: the bitonic network in its one-direction form (every merge opens
//   swd_sort_pass     with the flip i <-> i ^ (k - 1), then the strides k / 4 ... 1 as i <-> i ^ j; the smaller value always goes
//                     to the smaller index).  In that form a value of +inf at an index >= n never moves, so the padding to a
//                     power of two is virtual: an index >= n is read as +inf and never written, and ld >= n is all a row needs.
//                     The tile kernel keeps SWD_TILE floats (64 KB of the CU's 160 KB LDS: two workgroups per CU) and runs every
//                     compare-exchange that stays inside an aligned tile: the whole network up to k = SWD_TILE, and the strides
//                     SWD_TILE / 2 ... 1 of every later merge; the masks below 4 run in registers on 16-byte LDS accesses.  The
//                     pass kernel runs the steps that cross tiles over global memory, two masks per pass (a 4-element butterfly).
//   swd_absdiff       sum over rows r and i < n of |A[r][i] - B[r][i] + off[r]| (off: the per-row constant that the projection
//                     left out, 0 when null), every term formed and added in float64: a thread in column order, the wave by
//                     a butterfly, the waves in wave order, swd_final over the partials.  Columns >= n are never read.
// No atomics anywhere: two calls are bitwise equal.
#include "../../../include/contrad_hip.h"
#include "../common.h"

#include <math.h>

namespace {

constexpr int SWD_THREADS = 256;
constexpr int SWD_TILE_LOG = 14;
constexpr int SWD_TILE = 1 << SWD_TILE_LOG;          // floats of a sort tile in LDS
constexpr int SWD_SORT_THREADS = 1024;
constexpr int SWD_ABS_COLS = SWD_THREADS * 16;       // columns of a row that one workgroup of swd_absdiff adds
constexpr int SWD_DESC = 147, SWD_BANK_ROWS = 148;

__device__ __forceinline__ int mirror(int i, int R) {                // scipy's 'mirror' for |overhang| <= 2 < R
  i = i < 0 ? -i : i;
  return i >= R ? 2 * R - 2 - i : i;
}

__device__ __forceinline__ float gw(int d) {                         // 16 g[d + 2]
  return d == 0 ? 6.f : (d == 1 || d == -1) ? 4.f : 1.f;
}

__global__ __launch_bounds__(SWD_THREADS) void swd_u8_planes_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst,
                                                                    long long n, int R) {
  const long long total = n * 3 * R * R;
  const long long i = (long long)blockIdx.x * SWD_THREADS + threadIdx.x;
  if (i >= total) return;
  const long long hw = (long long)R * R;
  const long long plane = i / hw, p = i - plane * hw;
  const long long img = plane / 3;
  const int c = (int)(plane - img * 3);
  dst[i] = (float)src[(img * hw + p) * 3 + c];
}

__global__ __launch_bounds__(SWD_THREADS) void swd_pyr_down_kernel(const float* __restrict__ fine, float* __restrict__ coarse,
                                                                   long long planes, int R) {
  const int Rc = R >> 1;
  const long long total = planes * Rc * Rc;
  const long long i = (long long)blockIdx.x * SWD_THREADS + threadIdx.x;
  if (i >= total) return;
  const long long plane = i / ((long long)Rc * Rc);
  const int p = (int)(i - plane * Rc * Rc), y = p / Rc, x = p - y * Rc;
  const float* src = fine + plane * R * R;
  float acc = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const float* row = src + (long long)mirror(2 * y + dy, R) * R;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) acc += (gw(dy) * gw(dx) * (1.f / 256.f)) * row[mirror(2 * x + dx, R)];
  }
  coarse[i] = acc;
}

__global__ __launch_bounds__(SWD_THREADS) void swd_pyr_up_sub_kernel(float* __restrict__ fine, const float* __restrict__ coarse,
                                                                     long long planes, int R) {
  const int Rc = R >> 1;
  const long long total = planes * R * R;
  const long long i = (long long)blockIdx.x * SWD_THREADS + threadIdx.x;
  if (i >= total) return;
  const long long plane = i / ((long long)R * R);
  const int p = (int)(i - plane * R * R), y = p / R, x = p - y * R;
  const float* src = coarse + plane * Rc * Rc;
  float acc = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int yy = mirror(y + dy, R);
    if (yy & 1) continue;                                           // a zero of the zero-insert
    const float* row = src + (long long)(yy >> 1) * Rc;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int xx = mirror(x + dx, R);
      if (xx & 1) continue;
      acc += (gw(dy) * gw(dx) * (1.f / 64.f)) * row[xx >> 1];       // 4 g g / 256
    }
  }
  fine[i] -= acc;
}

// The wave's sum by a butterfly, the waves in wave order; the result is valid in thread 0.
__device__ __forceinline__ double block_sum64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(SWD_THREADS) void swd_gather_kernel(const float* __restrict__ level, int R, const int* __restrict__ cx,
                                                                 const int* __restrict__ cy, int nhoods, long long n_desc,
                                                                 long long n_pad, float* __restrict__ bank,
                                                                 double* __restrict__ partial) {
  __shared__ double red[4];
  const long long d = (long long)blockIdx.x * SWD_THREADS + threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
  if (d < n_desc) {
    const int x0 = min(max(cx[d], 3), R - 4) - 3, y0 = min(max(cy[d], 3), R - 4) - 3;
    const float* img = level + (d / nhoods) * 3 * R * R;
    for (int c = 0; c < 3; ++c)
      for (int dy = 0; dy < 7; ++dy) {
        const float* row = img + ((long long)c * R + (y0 + dy)) * R + x0;
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) {
          const float v = row[dx];
          bank[(long long)(c * 49 + dy * 7 + dx) * n_pad + d] = v;
          s[c] += (double)v;
          q[c] += (double)v * (double)v;                            // 24 x 24 bits: exact
        }
      }
    bank[(long long)SWD_DESC * n_pad + d] = 0.f;
  } else if (d < n_pad) {
    for (int r = 0; r < SWD_BANK_ROWS; ++r) bank[(long long)r * n_pad + d] = 0.f;
  }
  for (int c = 0; c < 3; ++c) {
    const double a = block_sum64(s[c], red);
    if (threadIdx.x == 0) partial[(long long)blockIdx.x * 6 + c] = a;
    const double b = block_sum64(q[c], red);
    if (threadIdx.x == 0) partial[(long long)blockIdx.x * 6 + 3 + c] = b;
  }
}

// out[j] (j = blockIdx.x < m) = the sum over b < nb of partial[b * m + j]: thread t the partials t, t + 256, ...; then a tree
// in LDS; one thread adds the old value last when `accumulate` is set.
__global__ __launch_bounds__(SWD_THREADS) void swd_final_kernel(const double* __restrict__ partial, long long nb, int m,
                                                                int accumulate, double* __restrict__ out) {
  __shared__ double red[SWD_THREADS];
  const int tid = threadIdx.x, j = blockIdx.x;
  double a = 0.0;
  for (long long i = tid; i < nb; i += SWD_THREADS) a += partial[i * m + j];
  red[tid] = a;
  __syncthreads();
  for (int s = SWD_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[j] = accumulate ? out[j] + red[0] : red[0];
}

__global__ __launch_bounds__(SWD_THREADS) void swd_absdiff_kernel(const float* __restrict__ A, long long ldA,
                                                                  const float* __restrict__ B, long long ldB,
                                                                  const double* __restrict__ off, int n, int chunks,
                                                                  double* __restrict__ partial) {
  __shared__ double red[4];
  const int r = blockIdx.x / chunks, ch = blockIdx.x - r * chunks;
  const float* a = A + (long long)r * ldA;
  const float* b = B + (long long)r * ldB;
  const double o = off ? off[r] : 0.0;
  const int c0 = ch * SWD_ABS_COLS + threadIdx.x;
  double acc = 0.0;
#pragma unroll 4
  for (int u = 0; u < 16; ++u) {
    const int c = c0 + u * SWD_THREADS;
    if (c < n) acc += fabs(((double)a[c] - (double)b[c]) + o);
  }
  acc = block_sum64(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// ---- the row sort ----
__device__ __forceinline__ void cmpx(float& lo, float& hi) {        // the smaller value to `lo`
  const float a = lo, b = hi;
  const bool sw = a > b;
  lo = sw ? b : a;
  hi = sw ? a : b;
}

// One step on the tile in LDS: the pairs (i, i ^ mask) with bit `hb` (the top bit of mask) of i clear.
__device__ __forceinline__ void tile_step(float* t, int mask, int hb_log) {
  for (int p = threadIdx.x; p < SWD_TILE / 2; p += SWD_SORT_THREADS) {
    const int i = ((p >> hb_log) << (hb_log + 1)) | (p & ((1 << hb_log) - 1));
    const int j = i ^ mask;                                          // j > i: bit hb_log is set in j alone
    float a = t[i], b = t[j];
    cmpx(a, b);
    t[i] = a;
    t[j] = b;
  }
  __syncthreads();
}

// The steps whose masks are below 4, on four neighbours in registers.  first: the network up to k = 4 (flip 1; flip 3,
// stride 1); otherwise the strides 2, 1 that close a merge.
__device__ __forceinline__ void tile_quads(float* t, bool first) {
  for (int p = threadIdx.x; p < SWD_TILE / 4; p += SWD_SORT_THREADS) {
    f32x4 v = *reinterpret_cast<f32x4*>(t + 4 * p);
    float a = v.x, b = v.y, c = v.z, d = v.w;
    if (first) {
      cmpx(a, b); cmpx(c, d);                                        // k = 2
      cmpx(a, d); cmpx(b, c);                                        // k = 4: the flip
      cmpx(a, b); cmpx(c, d);
    } else {
      cmpx(a, c); cmpx(b, d);
      cmpx(a, b); cmpx(c, d);
    }
    v.x = a; v.y = b; v.z = c; v.w = d;
    *reinterpret_cast<f32x4*>(t + 4 * p) = v;
  }
  __syncthreads();
}

// full: the whole network up to k = 2^kmax_log (<= SWD_TILE) on every aligned tile; otherwise the strides SWD_TILE / 2 ... 1
// of a later merge.  A tile that starts at or behind n holds +inf alone and is left.
__global__ __launch_bounds__(SWD_SORT_THREADS) void swd_sort_tile_kernel(float* __restrict__ X, long long ld, int n, int tiles,
                                                                         int full, int kmax_log) {
  __shared__ __attribute__((aligned(16))) float t[SWD_TILE];
  const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  const int base = tile * SWD_TILE;
  if (base >= n) return;                                             // (uniform)
  float* x = X + (long long)row * ld + base;
  const int live = min(SWD_TILE, n - base);
  for (int i = threadIdx.x; i < SWD_TILE; i += SWD_SORT_THREADS) t[i] = i < live ? x[i] : INFINITY;
  __syncthreads();
  if (full) {
    tile_quads(t, true);
    for (int k = 3; k <= kmax_log; ++k) {
      tile_step(t, (1 << k) - 1, k - 1);                             // the flip
      for (int j = k - 2; j >= 2; --j) tile_step(t, 1 << j, j);
      tile_quads(t, false);
    }
  } else {
    for (int j = SWD_TILE_LOG - 1; j >= 2; --j) tile_step(t, 1 << j, j);
    tile_quads(t, false);
  }
  for (int i = threadIdx.x; i < live; i += SWD_SORT_THREADS) x[i] = t[i];
}

// One pass over global memory: mask m1 (its top bit 2^b1), then, when m2 != 0, the stride m2 = 2^b2 (b2 < b1), on the four
// elements i, i ^ m2, i ^ m1, i ^ m1 ^ m2 of every i with the bits b1 and b2 clear (with m2 = 0: on the pair i, i ^ m1).
__global__ __launch_bounds__(SWD_THREADS) void swd_sort_pass_kernel(float* __restrict__ X, long long ld, int n, long long per_row,
                                                                    long long total, int m1, int b1, int m2, int b2) {
  const long long g = (long long)blockIdx.x * SWD_THREADS + threadIdx.x;
  if (g >= total) return;
  const long long row = g / per_row;
  long long p = g - row * per_row;
  float* x = X + row * ld;
  if (m2) p = ((p >> b2) << (b2 + 1)) | (p & ((1ll << b2) - 1));
  const long long i = ((p >> b1) << (b1 + 1)) | (p & ((1ll << b1) - 1));
  if (i >= n) return;                                                // the smallest index of the group: the rest is +inf too
  if (!m2) {
    const long long j = i ^ m1;
    if (j >= n) return;
    float a = x[i], b = x[j];
    cmpx(a, b);
    x[i] = a;
    x[j] = b;
    return;
  }
  const long long e0 = i, e1 = i ^ m2, e2 = i ^ m1, e3 = e2 ^ m2;     // e0 < e1, e0 < e2, e1 < e3
  float v0 = x[e0];
  float v1 = e1 < n ? x[e1] : INFINITY;
  float v2 = e2 < n ? x[e2] : INFINITY;
  float v3 = e3 < n ? x[e3] : INFINITY;
  cmpx(v0, v2);
  cmpx(v1, v3);
  cmpx(v0, v1);
  if (e2 < e3) cmpx(v2, v3); else cmpx(v3, v2);                      // (after a flip e3 lies below e2)
  x[e0] = v0;
  if (e1 < n) x[e1] = v1;
  if (e2 < n) x[e2] = v2;
  if (e3 < n) x[e3] = v3;
}

int ceil_log2(long long n) {
  int l = 0;
  while ((1ll << l) < n) ++l;
  return l;
}

}  // namespace

extern "C" int contrad_swd_sort_tile(void) { return SWD_TILE; }

extern "C" int contrad_swd_u8_planes(const void* src_u8, float* dst, long long n, int R, contrad_stream_t stream) {
  CONTRAD_ARG(src_u8 && dst);
  CONTRAD_ARG(n >= 1 && R >= 1 && R <= 32768);
  const long long total = n * 3 * R * R;
  CONTRAD_ARG(cdivll(total, SWD_THREADS) <= 0x7fffffffll);
  hipLaunchKernelGGL(swd_u8_planes_kernel, dim3((unsigned)cdivll(total, SWD_THREADS)), dim3(SWD_THREADS), 0, (hipStream_t)stream,
                     (const unsigned char*)src_u8, dst, n, R);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_swd_pyr_down(const float* fine, float* coarse, long long planes, int R, contrad_stream_t stream) {
  CONTRAD_ARG(fine && coarse && fine != coarse);
  CONTRAD_ARG(planes >= 1 && R >= 4 && R % 2 == 0 && R <= 32768);
  const long long total = planes * (R / 2) * (R / 2);
  CONTRAD_ARG(cdivll(total, SWD_THREADS) <= 0x7fffffffll);
  hipLaunchKernelGGL(swd_pyr_down_kernel, dim3((unsigned)cdivll(total, SWD_THREADS)), dim3(SWD_THREADS), 0, (hipStream_t)stream,
                     fine, coarse, planes, R);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_swd_pyr_up_sub(float* fine, const float* coarse, long long planes, int R, contrad_stream_t stream) {
  CONTRAD_ARG(fine && coarse && fine != coarse);
  CONTRAD_ARG(planes >= 1 && R >= 4 && R % 2 == 0 && R <= 32768);
  const long long total = planes * R * R;
  CONTRAD_ARG(cdivll(total, SWD_THREADS) <= 0x7fffffffll);
  hipLaunchKernelGGL(swd_pyr_up_sub_kernel, dim3((unsigned)cdivll(total, SWD_THREADS)), dim3(SWD_THREADS), 0, (hipStream_t)stream,
                     fine, coarse, planes, R);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" long long contrad_swd_gather_workspace_bytes(long long n_desc) {
  if (n_desc < 1 || cdivll(n_desc + 3, SWD_THREADS) > 0x7fffffffll) return -22;
  return cdivll((n_desc + 3) / 4 * 4, SWD_THREADS) * 6 * (long long)sizeof(double);
}

extern "C" int contrad_swd_gather(const float* level, long long n_images, int R, const int* cx, const int* cy, int nhoods,
                                  float* bank, long long n_pad, double* stats, void* workspace, long long workspace_bytes,
                                  contrad_stream_t stream) {
  CONTRAD_ARG(level && cx && cy && bank && stats);
  CONTRAD_ARG(n_images >= 1 && n_images <= 0x7fffffffll && nhoods >= 1 && nhoods <= (1 << 20) && R >= 7 && R <= 32768);
  const long long n_desc = n_images * nhoods;
  CONTRAD_ARG(n_pad == (n_desc + 3) / 4 * 4);
  const long long need = contrad_swd_gather_workspace_bytes(n_desc);
  CONTRAD_ARG(need > 0 && workspace && workspace_bytes >= need);
  CONTRAD_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0);
  const long long blocks = cdivll(n_pad, SWD_THREADS);
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(swd_gather_kernel, dim3((unsigned)blocks), dim3(SWD_THREADS), 0, st, level, R, cx, cy, nhoods, n_desc,
                     n_pad, bank, partial);
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(swd_final_kernel, dim3(6), dim3(SWD_THREADS), 0, st, partial, blocks, 6, 0, stats);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_swd_sort_rows(float* X, long long ld, int rows, int n, contrad_stream_t stream) {
  CONTRAD_ARG(X);
  CONTRAD_ARG(rows >= 1 && n >= 1 && ld >= n && n <= (1 << 30));
  hipStream_t st = (hipStream_t)stream;
  const int plog = ceil_log2(n);                                     // the network's length 2^plog >= n
  const int tiles = (int)cdivll(n, SWD_TILE);
  CONTRAD_ARG((long long)rows * tiles <= 0x7fffffffll);
  const dim3 tgrid((unsigned)((long long)rows * tiles));
  if (plog == 0) return 0;
  hipLaunchKernelGGL(swd_sort_tile_kernel, tgrid, dim3(SWD_SORT_THREADS), 0, st, X, ld, n, tiles, 1,
                     plog < 2 ? 2 : (plog < SWD_TILE_LOG ? plog : SWD_TILE_LOG));
  CONTRAD_CHECK_LAUNCH();
  for (int k = SWD_TILE_LOG + 1; k <= plog; ++k) {
    // the masks of this merge that cross tiles: the flip 2^k - 1, then the strides 2^(k-2) ... SWD_TILE
    int masks[32], bits[32], nm = 0;
    masks[nm] = (int)((1ll << k) - 1); bits[nm++] = k - 1;
    for (int j = k - 2; j >= SWD_TILE_LOG; --j) { masks[nm] = 1 << j; bits[nm++] = j; }
    for (int s = 0; s < nm; s += 2) {
      const bool two = s + 1 < nm;
      const long long per_row = (1ll << plog) >> (two ? 2 : 1);
      const long long total = per_row * rows;
      CONTRAD_ARG(cdivll(total, SWD_THREADS) <= 0x7fffffffll);
      hipLaunchKernelGGL(swd_sort_pass_kernel, dim3((unsigned)cdivll(total, SWD_THREADS)), dim3(SWD_THREADS), 0, st, X, ld, n,
                         per_row, total, masks[s], bits[s], two ? masks[s + 1] : 0, two ? bits[s + 1] : 0);
      CONTRAD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(swd_sort_tile_kernel, tgrid, dim3(SWD_SORT_THREADS), 0, st, X, ld, n, tiles, 0, SWD_TILE_LOG);
    CONTRAD_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" long long contrad_swd_absdiff_workspace_bytes(int rows, int n) {
  if (rows < 1 || n < 1 || n > (1 << 30)) return -22;
  const long long blocks = (long long)rows * cdivll(n, SWD_ABS_COLS);
  if (blocks > 0x7fffffffll) return -22;
  return blocks * (long long)sizeof(double);
}

extern "C" int contrad_swd_absdiff_sums(const float* A, long long ldA, const float* B, long long ldB, const double* row_offset,
                                        int rows, int n, int accumulate, double* out, void* workspace,
                                        long long workspace_bytes, contrad_stream_t stream) {
  CONTRAD_ARG(A && B && out);
  CONTRAD_ARG(rows >= 1 && n >= 1 && ldA >= n && ldB >= n);
  const long long need = contrad_swd_absdiff_workspace_bytes(rows, n);
  CONTRAD_ARG(need > 0 && workspace && workspace_bytes >= need);
  CONTRAD_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)row_offset & 7) == 0);
  const int chunks = (int)cdivll(n, SWD_ABS_COLS);
  const long long blocks = (long long)rows * chunks;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(swd_absdiff_kernel, dim3((unsigned)blocks), dim3(SWD_THREADS), 0, st, A, ldA, B, ldB, row_offset, n, chunks,
                     partial);
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(swd_final_kernel, dim3(1), dim3(SWD_THREADS), 0, st, partial, blocks, 1, accumulate ? 1 : 0, out);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
