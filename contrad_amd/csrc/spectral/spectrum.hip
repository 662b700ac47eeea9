// Radial power spectrum of uint8 images (gfx950): the device side of contrad_amd/spectrum.py.
//
//   spec_rfft2_*      uint8 NHWC [n][S][S][3] -> the half spectrum spec[n][S][S/2 + 1] (complex fp32, numpy.fft.rfft2's layout)
//                     of the exact luma Y = (77 R + 150 G + 29 B) / 256.  A register FFT with LDS exchanges: decimation in
//                     time on bit-reversed input, two radix-2 stages per LDS round trip (four points per thread in
//                     registers), one last radix-2 stage when log2 S is odd.  The twiddles are the caller's fp32 table
//                     (cos, -sin)(2 pi j / S), j < S / 2, copied to LDS; stages 0 and 1 use 1 and -i as sign swaps, not
//                     products.  No sincosf, no fast-math intrinsic.
//                     Two real rows 2p, 2p + 1 are one complex row FFT z = row_2p + i row_2p+1 and come apart by symmetry:
//                     A[v] = (Z[v] + conj Z[S - v]) / 2, B[v] = (Z[v] - conj Z[S - v]) / 2i.
//                     S <= 128 (fused): a workgroup keeps the packed rows (S/2 x S complex) and the half spectrum, stored
//                     column-major with a row stride of S + 1 (odd in 8-byte units: the transposing writes and reads of a
//                     wave fall on distinct banks), in LDS together: 130 KB at S = 128.  16 images per workgroup at
//                     S = 16, 4 at S = 32, 1 above; images behind n are read as zero and not stored.
//                     S = 256, 512 (two passes): the row kernel transforms 8 row pairs per workgroup and writes the
//                     separated rows to spec; the column kernel transforms 16 columns x S rows in place on spec through an
//                     LDS tile of the same padded layout, so that global accesses are 128-byte runs along v; the last
//                     tile of an image also takes the odd column v = S / 2 (no workgroup runs for one column).
//                     Why not a matrix-product DFT on the fp32 MFMAs: its rounding chain grows with S (2 S + 8 against
//                     15 log2 S - 22 here), and fp32 MFMA runs at the vector rate on this chip, so it buys no time.
//   spec_radial       prof[i][k] = rcount[k] / S^4 * sum over the members (u, v) of bin k on the half spectrum of
//                     w(v) |spec[i][u][v]|^2, w = 1 at v = 0 and v = S / 2 and 2 elsewhere, in float64.  One thread owns one
//                     (image, bin): bin_of is non-decreasing along v and along |fu|, so the members of bin k in row |fu| = a
//                     are one run [lo, hi) whose ends only move down as a grows; the owner walks a = 0 ... min(k, S / 2),
//                     row u = a then row u = S - a, v ascending.  No square root on the device.
//   spec_mean_map     map[u][v] (+)= 1 / S^4 * sum over the images of |spec[i][u][v]|^2 in float64.  Each entry has one
//                     owner row of G threads (G = 1, 4, 16 or 64 by S alone: small maps have too few entries to fill the
//                     chip); thread g adds the images g, g + G, ... in image order, thread 0 adds the G partials in order.
// Every buffer is an output: no scratch.  No atomics anywhere: two calls are bitwise equal.
#include "../../../include/contrad_hip.h"
#include "../common.h"

#include <stdint.h>

namespace {

constexpr int SPEC_ROW_PAIRS = 8;        // row pairs per workgroup of the row kernel
constexpr int SPEC_COL_TILE = 16;        // columns per workgroup of the column kernel: 128 bytes along v
constexpr int SPEC_RADIAL_THREADS = 128;

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

template <int K>
__device__ __forceinline__ int bitrev(int x) { return (int)(__brev((unsigned)x) >> (32 - K)); }

// nfft transforms of length S = 2^K in place, transform f at a + f * stride, input in bit-reversed order, output in natural
// order.  tw[j] = exp(-2 pi i j / S), j < S / 2.  Every thread of the workgroup must call it; it ends with a barrier.
template <int K, int THREADS>
__device__ __forceinline__ void fft_lds(float2* a, int nfft, int stride, const float2* tw) {
  constexpr int S = 1 << K, Q = S / 4;
#pragma unroll
  for (int s = 0; s + 1 < K; s += 2) {
    const int h = 1 << s;
    for (int w = threadIdx.x; w < nfft * Q; w += THREADS) {
      const int f = w >> (K - 2), q = w & (Q - 1);
      const int j = q & (h - 1);
      float2* p = a + f * stride + (((q >> s) << (s + 2)) | j);
      float2 x0 = p[0], x1 = p[h], x2 = p[2 * h], x3 = p[3 * h];
      if (s > 0) {
        const float2 w1 = tw[j << (K - 1 - s)];
        x1 = cmul(x1, w1);
        x3 = cmul(x3, w1);
      }
      const float2 y0 = cadd(x0, x1), y1 = csub(x0, x1);
      float2 y2 = cadd(x2, x3), y3 = csub(x2, x3);
      if (s > 0) {
        y2 = cmul(y2, tw[j << (K - 2 - s)]);
        y3 = cmul(y3, tw[(j + h) << (K - 2 - s)]);
      } else {
        y3 = make_float2(y3.y, -y3.x);                               // times -i
      }
      p[0] = cadd(y0, y2);
      p[2 * h] = csub(y0, y2);
      p[h] = cadd(y1, y3);
      p[3 * h] = csub(y1, y3);
    }
    __syncthreads();
  }
  if (K & 1) {
    constexpr int h = S / 2;
    for (int w = threadIdx.x; w < nfft * h; w += THREADS) {
      const int f = w >> (K - 1), j = w & (h - 1);
      float2* p = a + f * stride + j;
      const float2 x0 = p[0], x1 = cmul(p[h], tw[j]);
      p[0] = cadd(x0, x1);
      p[h] = csub(x0, x1);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ float luma(unsigned r, unsigned g, unsigned b) {
  return (float)(int)(77u * r + 150u * g + 29u * b) * (1.f / 256.f);     // at most 65 280: exact
}

// The lumas of the four pixels that the three little-endian words w0, w1, w2 hold.
__device__ __forceinline__ void luma4(unsigned w0, unsigned w1, unsigned w2, float* y) {
  y[0] = luma(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
  y[1] = luma(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
  y[2] = luma((w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
  y[3] = luma((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
}

// Rows [0, 2 * pairs) of S pixels at `words` (null: zeros) into Z[pair][bitrev(x)], the even row as the real part.
template <int K, int THREADS>
__device__ __forceinline__ void load_packed_rows(const unsigned* __restrict__ words, int pairs, float* zf) {
  constexpr int S = 1 << K;
  for (int g = threadIdx.x; g < pairs * 2 * S / 4; g += THREADS) {
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    if (words) luma4(words[3 * g], words[3 * g + 1], words[3 * g + 2], y);
    const int p0 = 4 * g, row = p0 >> K, x = p0 & (S - 1);
    float* z = zf + (size_t)(row >> 1) * S * 2 + (row & 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) z[2 * bitrev<K>(x + i)] = y[i];
  }
}

// The two real rows' spectra at v from the packed transform Z of one pair.
template <int K>
__device__ __forceinline__ void separate(const float2* z, int v, float2& A, float2& B) {
  constexpr int S = 1 << K;
  const float2 zv = z[v & (S - 1)], zm = z[(S - v) & (S - 1)];
  A = make_float2(0.5f * (zv.x + zm.x), 0.5f * (zv.y - zm.y));
  B = make_float2(0.5f * (zv.y + zm.y), -0.5f * (zv.x - zm.x));
}

template <int K, int IMGS>
constexpr size_t fused_lds() {
  return sizeof(float2) * ((size_t)(1 << K) / 2 + (size_t)IMGS * ((1 << K) / 2) * (1 << K) +
                           (size_t)IMGS * ((1 << K) / 2 + 1) * ((1 << K) + 1));
}

template <int K, int IMGS, int THREADS>
__global__ __launch_bounds__(THREADS) void spec_rfft2_fused_kernel(const unsigned char* __restrict__ src,
                                                                   const float2* __restrict__ tw_g, float2* __restrict__ spec,
                                                                   long long n) {
  constexpr int S = 1 << K, HS = S / 2 + 1, CS = S + 1;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  float2* tw = lds;                                  // [S / 2]
  float2* Z = tw + S / 2;                            // [IMGS][S / 2][S]
  float2* Hc = Z + IMGS * (S / 2) * S;               // [IMGS][HS][CS]: column v of image im at (im * HS + v) * CS
  const long long img0 = (long long)blockIdx.x * IMGS;
  for (int j = threadIdx.x; j < S / 2; j += THREADS) tw[j] = tw_g[j];
  for (int im = 0; im < IMGS; ++im) {
    const unsigned* words = img0 + im < n ? reinterpret_cast<const unsigned*>(src + (img0 + im) * 3 * S * S) : nullptr;
    load_packed_rows<K, THREADS>(words, S / 2, reinterpret_cast<float*>(Z + im * (S / 2) * S));
  }
  __syncthreads();
  fft_lds<K, THREADS>(Z, IMGS * (S / 2), S, tw);
  for (int e = threadIdx.x; e < IMGS * (S / 2) * HS; e += THREADS) {
    const int f = e / HS, v = e - f * HS;             // f = im * (S / 2) + pair
    const int im = f >> (K - 1), p = f & (S / 2 - 1);
    float2 A, B;
    separate<K>(Z + f * S, v, A, B);
    float2* col = Hc + (im * HS + v) * CS;
    col[bitrev<K>(2 * p)] = A;
    col[bitrev<K>(2 * p + 1)] = B;
  }
  __syncthreads();
  fft_lds<K, THREADS>(Hc, IMGS * HS, CS, tw);
  for (int e = threadIdx.x; e < IMGS * S * HS; e += THREADS) {
    const int im = e / (S * HS), r = e - im * (S * HS);
    const int u = r / HS, v = r - u * HS;
    if (img0 + im < n) spec[(img0 + im) * (S * HS) + r] = Hc[(im * HS + v) * CS + u];
  }
}

template <int K, int THREADS>
__global__ __launch_bounds__(THREADS) void spec_rfft2_rows_kernel(const unsigned char* __restrict__ src,
                                                                  const float2* __restrict__ tw_g, float2* __restrict__ spec) {
  constexpr int S = 1 << K, HS = S / 2 + 1, RP = SPEC_ROW_PAIRS, GROUPS = S / 2 / RP;
  __shared__ __attribute__((aligned(16))) float2 tw[S / 2];
  __shared__ __attribute__((aligned(16))) float2 Z[RP * S];
  const long long img = blockIdx.x / GROUPS;
  const int y0 = (int)(blockIdx.x - img * GROUPS) * RP * 2;
  for (int j = threadIdx.x; j < S / 2; j += THREADS) tw[j] = tw_g[j];
  load_packed_rows<K, THREADS>(reinterpret_cast<const unsigned*>(src + (img * S + y0) * 3 * S), RP, reinterpret_cast<float*>(Z));
  __syncthreads();
  fft_lds<K, THREADS>(Z, RP, S, tw);
  float2* out = spec + (img * S + y0) * HS;
  for (int e = threadIdx.x; e < RP * HS; e += THREADS) {
    const int p = e / HS, v = e - p * HS;
    float2 A, B;
    separate<K>(Z + p * S, v, A, B);
    out[(2 * p) * HS + v] = A;
    out[(2 * p + 1) * HS + v] = B;
  }
}

template <int K>
constexpr size_t cols_lds() { return sizeof(float2) * ((size_t)(1 << K) / 2 + (size_t)(SPEC_COL_TILE + 1) * ((1 << K) + 1)); }

template <int K, int THREADS>
__global__ __launch_bounds__(THREADS) void spec_rfft2_cols_kernel(const float2* __restrict__ tw_g, float2* __restrict__ spec) {
  constexpr int S = 1 << K, HS = S / 2 + 1, CS = S + 1, CT = SPEC_COL_TILE, TILES = (S / 2) / CT;
  static_assert((S / 2) % CT == 0, "the columns 0 ... S / 2 - 1 are whole tiles");
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  float2* tw = lds;                                  // [S / 2]
  float2* C = tw + S / 2;                            // [CT + 1][CS]: the last tile of an image also takes the column S / 2
  const long long img = blockIdx.x / TILES;
  const int tile = (int)(blockIdx.x - img * TILES);
  const bool extra = tile == TILES - 1;              // (uniform over the workgroup)
  float2* sp = spec + img * S * HS + tile * CT;
  for (int j = threadIdx.x; j < S / 2; j += THREADS) tw[j] = tw_g[j];
  for (int e = threadIdx.x; e < S * CT; e += THREADS) {
    const int u = e / CT, c = e - u * CT;
    C[c * CS + bitrev<K>(u)] = sp[(long long)u * HS + c];
  }
  if (extra)
    for (int u = threadIdx.x; u < S; u += THREADS) C[CT * CS + bitrev<K>(u)] = sp[(long long)u * HS + CT];
  __syncthreads();
  fft_lds<K, THREADS>(C, extra ? CT + 1 : CT, CS, tw);
  for (int e = threadIdx.x; e < S * CT; e += THREADS) {
    const int u = e / CT, c = e - u * CT;
    sp[(long long)u * HS + c] = C[c * CS + u];
  }
  if (extra)
    for (int u = threadIdx.x; u < S; u += THREADS) sp[(long long)u * HS + CT] = C[CT * CS + u];
}

__device__ __forceinline__ double power64(float2 z) {
  return (double)z.x * (double)z.x + (double)z.y * (double)z.y;     // 24 x 24 bits: both squares exact
}

__global__ __launch_bounds__(SPEC_RADIAL_THREADS) void spec_radial_kernel(const float2* __restrict__ spec,
                                                                          const int* __restrict__ bin_of,
                                                                          const double* __restrict__ rcount,
                                                                          double* __restrict__ prof, long long total, int S,
                                                                          int K, double inv_s4) {
  const long long g = (long long)blockIdx.x * SPEC_RADIAL_THREADS + threadIdx.x;
  if (g >= total) return;
  const long long img = g / K;
  const int k = (int)(g - img * K);
  const int half = S >> 1, HS = half + 1;
  const float2* sp = spec + img * S * HS;
  int lo = HS, hi = HS;                                               // the members of bin k in row a: [lo, hi)
  double acc = 0.0;
  const int last = k < half ? k : half;                               // bin_of[a][v] >= a: nothing of bin k behind row k
  for (int a = 0; a <= last; ++a) {
    const int* row = bin_of + (long long)a * HS;
    while (lo > 0 && row[lo - 1] >= k) --lo;
    while (hi > 0 && row[hi - 1] > k) --hi;
    const int reps = (a == 0 || a == half) ? 1 : 2;
    for (int rep = 0; rep < reps; ++rep) {
      const float2* r = sp + (long long)(rep ? S - a : a) * HS;
      for (int v = lo; v < hi; ++v) {
        const double p = power64(r[v]);
        acc += (v == 0 || v == half) ? p : 2.0 * p;
      }
    }
  }
  prof[g] = acc * rcount[k] * inv_s4;
}

__global__ void spec_mean_map_kernel(const float2* __restrict__ spec, double* __restrict__ map, long long n, long long E,
                                     int accumulate, double inv_s4) {
  extern __shared__ __attribute__((aligned(16))) double part[];       // [G][ENT]
  const int ENT = blockDim.x, G = blockDim.y, tx = threadIdx.x, g = threadIdx.y;
  const long long e = (long long)blockIdx.x * ENT + tx;
  double acc = 0.0;
  if (e < E) {
#pragma unroll 4
    for (long long i = g; i < n; i += G) acc += power64(spec[i * E + e]);
  }
  part[g * ENT + tx] = acc;
  __syncthreads();
  if (g == 0 && e < E) {
    double s = part[tx];
    for (int j = 1; j < G; ++j) s += part[j * ENT + tx];
    s *= inv_s4;
    map[e] = accumulate ? map[e] + s : s;
  }
}

// Raise a kernel's dynamic LDS limit once per device (one process may drive several; benign race: idempotent); a failure is
// returned and tried again by the next call.
int allow_lds(const void* kernel, size_t lds_bytes, bool (&done)[64]) {
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  bool& set = done[dev_id & 63];
  if (!set) {
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    set = true;
  }
  return 0;
}

int log2_of_side(int S) {                                             // 4 ... 9 for 16 ... 512, else 0
  for (int k = 4; k <= 9; ++k)
    if (S == (1 << k)) return k;
  return 0;
}

template <int K, int IMGS, int THREADS>
int launch_fused(const unsigned char* src, const float2* tw, float2* spec, long long n, hipStream_t st) {
  constexpr size_t lds = fused_lds<K, IMGS>();
  static bool done[64] = {};
  const int rc = allow_lds(reinterpret_cast<const void*>(&spec_rfft2_fused_kernel<K, IMGS, THREADS>), lds, done);
  if (rc != 0) return rc;
  hipLaunchKernelGGL((spec_rfft2_fused_kernel<K, IMGS, THREADS>), dim3((unsigned)cdivll(n, IMGS)), dim3(THREADS), lds, st, src, tw,
                     spec, n);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

template <int K, int THREADS>
int launch_two_pass(const unsigned char* src, const float2* tw, float2* spec, long long n, hipStream_t st) {
  constexpr int S = 1 << K, HS = S / 2 + 1;
  constexpr size_t lds = cols_lds<K>();
  static bool done[64] = {};
  const int rc = allow_lds(reinterpret_cast<const void*>(&spec_rfft2_cols_kernel<K, THREADS>), lds, done);
  if (rc != 0) return rc;
  hipLaunchKernelGGL((spec_rfft2_rows_kernel<K, THREADS>), dim3((unsigned)(n * (S / 2 / SPEC_ROW_PAIRS))), dim3(THREADS), 0, st, src,
                     tw, spec);
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL((spec_rfft2_cols_kernel<K, THREADS>), dim3((unsigned)(n * ((S / 2) / SPEC_COL_TILE))), dim3(THREADS), lds, st, tw,
                     spec);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int contrad_spec_rfft2(const void* src_u8, const float* twiddles, float* spec, long long n, int S,
                                  contrad_stream_t stream) {
  CONTRAD_ARG(src_u8 && twiddles && spec);
  const int K = log2_of_side(S);
  CONTRAD_ARG(K != 0 && n >= 1 && n <= (1ll << 24));                  // (2^24 images x 64 blocks: the grid stays below 2^31)
  CONTRAD_ARG(((uintptr_t)src_u8 & 3) == 0 && ((uintptr_t)twiddles & 7) == 0 && ((uintptr_t)spec & 7) == 0);
  const unsigned char* src = (const unsigned char*)src_u8;
  const float2* tw = (const float2*)twiddles;
  float2* out = (float2*)spec;
  hipStream_t st = (hipStream_t)stream;
  switch (K) {
    case 4: return launch_fused<4, 16, 256>(src, tw, out, n, st);
    case 5: return launch_fused<5, 4, 256>(src, tw, out, n, st);
    case 6: return launch_fused<6, 1, 256>(src, tw, out, n, st);
    case 7: return launch_fused<7, 1, 512>(src, tw, out, n, st);
    case 8: return launch_two_pass<8, 256>(src, tw, out, n, st);
    default: return launch_two_pass<9, 256>(src, tw, out, n, st);
  }
}

extern "C" int contrad_spec_radial(const float* spec, const int* bin_of, const double* rcount, double* prof, long long n, int S,
                                   int K, contrad_stream_t stream) {
  CONTRAD_ARG(spec && bin_of && rcount && prof);
  CONTRAD_ARG(log2_of_side(S) != 0 && n >= 1 && n <= (1ll << 24));
  CONTRAD_ARG(K >= S / 2 + 1 && K <= S);                              // (kmax = round(S / sqrt 2) lies between)
  CONTRAD_ARG(((uintptr_t)spec & 7) == 0 && ((uintptr_t)bin_of & 3) == 0 && ((uintptr_t)rcount & 7) == 0 && ((uintptr_t)prof & 7) == 0);
  const long long total = n * K;
  CONTRAD_ARG(cdivll(total, SPEC_RADIAL_THREADS) <= 0x7fffffffll);
  const double s2 = (double)S * (double)S;
  hipLaunchKernelGGL(spec_radial_kernel, dim3((unsigned)cdivll(total, SPEC_RADIAL_THREADS)), dim3(SPEC_RADIAL_THREADS), 0,
                     (hipStream_t)stream, (const float2*)spec, bin_of, rcount, prof, total, S, K, 1.0 / (s2 * s2));
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_spec_mean_map(const float* spec, double* map, long long n, int S, int accumulate,
                                     contrad_stream_t stream) {
  CONTRAD_ARG(spec && map);
  CONTRAD_ARG(log2_of_side(S) != 0 && n >= 1 && n <= (1ll << 24));
  CONTRAD_ARG(accumulate == 0 || accumulate == 1);
  CONTRAD_ARG(((uintptr_t)spec & 7) == 0 && ((uintptr_t)map & 7) == 0);
  const long long E = (long long)S * (S / 2 + 1);
  int G = 1;
  while (G < 64 && E * G < 65536) G *= 4;                             // 64, 64, 64, 16, 4, 1 for S = 16 ... 512
  const int ENT = 256 / G > 16 ? 256 / G : 16;
  const double s2 = (double)S * (double)S;
  hipLaunchKernelGGL(spec_mean_map_kernel, dim3((unsigned)cdivll(E, ENT)), dim3(ENT, G), (size_t)G * ENT * sizeof(double),
                     (hipStream_t)stream, (const float2*)spec, map, n, E, accumulate, 1.0 / (s2 * s2));
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
