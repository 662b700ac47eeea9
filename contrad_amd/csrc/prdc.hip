// Precision / recall / density / coverage on a similarity matrix (gfx950): the two selection kernels of
// contrad_amd/prdc.py.  Integer counts only: no float atomics, every sum is independent of the order of arrival, so two
// calls are bitwise equal.  The key order, the radix select, the round scan and the row-tile walk are csrc/simrow.h's
// (shared with knn.hip and kid.hip); this file owns:
//
//   prdc_kth     per row the k-th largest value with the column self0 + row left out: the radix select alone, so k is
//                bound by the row only.  A key names its float except for the two keys that several bit patterns share
//                (zero: -0.0 / +0.0; NaN): there one more ordered pass finds the column that holds the k-th place under
//                "value descending, column ascending" and its float is written.  One 256-thread workgroup per row.
//   prdc_count   one pass over S against a threshold per column (hit_c) and / or per row (hit_r), on row tiles of 128
//                rows x 256 columns.  Row counts: ballots summed per wave, one lane per row keeps the count, one global
//                add per row and tile.  Column counts: per-lane registers over the wave's rows, the four waves summed in
//                LDS, one global add per column and tile.  Zero sums are not sent.
#include "../../include/contrad_hip.h"
#include "simrow.h"

namespace {

constexpr int PRDC_THREADS = simrow::THREADS;
constexpr int PRDC_COLS = simrow::COLS;
constexpr int PRDC_RPW = 32;                        // rows per wave of a count tile
constexpr int PRDC_ROWS = 4 * PRDC_RPW;

__global__ __launch_bounds__(PRDC_THREADS) void prdc_kth_kernel(const float* __restrict__ S, long long ldS, int n, int k,
                                                                long long self0, float* __restrict__ thr) {
  __shared__ unsigned hist[4][256];
  __shared__ unsigned wtot[2][4];
  __shared__ unsigned sel[2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long q = blockIdx.x;
  const float* __restrict__ row = S + q * ldS;
  const unsigned un = (unsigned)n;
  const long long self = self0 >= 0 ? self0 + q : -1;
  const unsigned excl = (self >= 0 && self < (long long)n) ? (unsigned)self : 0xffffffffu;      // (n < 2^31: no column)

  // ---- the k-th largest key T; the k-th place is the `krem`-th of the columns equal to it ----
  unsigned krem = (unsigned)k;
  const unsigned T = simrow::kth_key<true, 1, 4>(row, un, excl, hist, wtot, sel, krem);

  if (T != 0u && T != 0x80000000u) {                   // one bit pattern has this key: the float itself
    if (tid == 0) thr[q] = __uint_as_float((T & 0x80000000u) ? (T & 0x7fffffffu) : ~T);
    return;
  }
  // ---- zero or NaN: the krem-th column equal to T in column order holds the k-th place ----
  unsigned base = 0u;
  int buf = 0;
  for (unsigned c0 = 0u; c0 < un; c0 += simrow::CHUNK, buf ^= 1) {
    const unsigned j0 = c0 + 4u * tid;
    unsigned e = 0u, mask = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned j = j0 + i;
      if (j < un && j != excl && simrow::key(row[j]) == T) {
        ++e;
        mask |= 1u << i;
      }
    }
    unsigned tot;
    const unsigned before = base + simrow::round_scan(e, wtot[buf], tot);
    if (before < krem && krem <= before + e) {         // exactly one thread of one round
      unsigned need = krem - before;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (((mask >> i) & 1u) && --need == 0u) thr[q] = row[j0 + i];
    }
    base += tot;
    if (base >= krem) break;                           // (uniform)
  }
}

template <bool HC, bool HR>
__global__ __launch_bounds__(PRDC_THREADS) void prdc_count_kernel(const float* __restrict__ S, long long ldS, int M, int n,
                                                                  const float* __restrict__ thr_row,
                                                                  const float* __restrict__ thr_col,
                                                                  int* __restrict__ row_hits, int* __restrict__ col_hits_c,
                                                                  int* __restrict__ col_hits_r, int ctiles, int vec_ok) {
  __shared__ int cs[2][4][PRDC_COLS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ct = blockIdx.x % ctiles, rt = blockIdx.x / ctiles;
  const long long tile_c0 = (long long)ct * PRDC_COLS, c0 = tile_c0 + 4 * lane;
  const int r0 = rt * PRDC_ROWS + w;                   // this wave's rows: r0, r0 + 4, ...
  const int rows = r0 < M ? min(PRDC_RPW, (M - r0 + 3) >> 2) : 0;
  const float nanf_ = __uint_as_float(0x7fc00000u);    // a column outside [0, n) hits nothing

  float tc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) tc[i] = (HC && c0 + i < n) ? thr_col[c0 + i] : nanf_;
  int cc[4] = {0, 0, 0, 0}, cr[4] = {0, 0, 0, 0}, mine = 0;
  for (int t0 = 0; t0 < rows; t0 += 4) {
    float v[4][4], tr[4];
    simrow::load_tile(v, S, ldS, r0, t0, rows, c0, n, vec_ok, nanf_,
                      [&](int u, long long i) __attribute__((always_inline)) { tr[u] = HR ? thr_row[i] : nanf_; });
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool live = t0 + u < rows;                 // (uniform)
      if (HC) {
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool h = live && v[u][j] >= tc[j];     // false on a NaN on either side
          cc[j] += h ? 1 : 0;
          cnt += __popcll(__ballot(h));
        }
        if (lane == t0 + u) mine = cnt;
      }
      if (HR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) cr[j] += (live && v[u][j] >= tr[u]) ? 1 : 0;
      }
    }
  }
  if (HC && lane < rows && mine != 0) atomicAdd(&row_hits[r0 + 4 * lane], mine);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (HC) cs[0][w][4 * lane + j] = cc[j];
    if (HR) cs[1][w][4 * lane + j] = cr[j];
  }
  __syncthreads();
  if (tile_c0 + tid < n) {
    if (HC) {
      const int s = cs[0][0][tid] + cs[0][1][tid] + cs[0][2][tid] + cs[0][3][tid];
      if (s != 0) atomicAdd(&col_hits_c[tile_c0 + tid], s);
    }
    if (HR) {
      const int s = cs[1][0][tid] + cs[1][1][tid] + cs[1][2][tid] + cs[1][3][tid];
      if (s != 0) atomicAdd(&col_hits_r[tile_c0 + tid], s);
    }
  }
}

}  // namespace

extern "C" int contrad_prdc_kth(const float* S, long long ldS, int M, int n, int k, long long self0, float* thr,
                                contrad_stream_t stream) {
  CONTRAD_ARG(S && thr);
  CONTRAD_ARG(M >= 1 && n >= 1 && ldS >= n);
  const int remain = (self0 >= 0 && self0 < n) ? n - 1 : n;         // the shortest row of the chunk
  CONTRAD_ARG(k >= 1 && k <= remain);
  hipLaunchKernelGGL(prdc_kth_kernel, dim3(M), dim3(PRDC_THREADS), 0, (hipStream_t)stream, S, ldS, n, k, self0, thr);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_prdc_count(const float* S, long long ldS, int M, int n, const float* thr_row, const float* thr_col,
                                  int* row_hits, int* col_hits_c, int* col_hits_r, contrad_stream_t stream) {
  CONTRAD_ARG(S && (thr_row || thr_col));
  CONTRAD_ARG(M >= 1 && n >= 1 && ldS >= n);
  CONTRAD_ARG(!thr_col || (row_hits && col_hits_c));
  CONTRAD_ARG(!thr_row || col_hits_r);
  const long long ctiles = cdivll(n, PRDC_COLS), blocks = ctiles * cdivll(M, PRDC_ROWS);
  CONTRAD_ARG(blocks <= 0x7fffffffll && M <= 0x7fffffff - PRDC_ROWS);
  const int vec_ok = (ldS % 4 == 0 && ((uintptr_t)S & 15) == 0) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (thr_col) {                                       // row_hits is written: zeroed here, added to per column tile
    const hipError_t e = hipMemsetAsync(row_hits, 0, sizeof(int) * (size_t)M, st);
    if (e != hipSuccess) return (int)e;
  }
#define PRDC_LAUNCH(HC, HR)                                                                                          \
  hipLaunchKernelGGL((prdc_count_kernel<HC, HR>), dim3((unsigned)blocks), dim3(PRDC_THREADS), 0, st, S, ldS, M, n, \
                     thr_row, thr_col, row_hits, col_hits_c, col_hits_r, (int)ctiles, vec_ok)
  if (thr_col && thr_row) PRDC_LAUNCH(true, true);
  else if (thr_col) PRDC_LAUNCH(true, false);
  else PRDC_LAUNCH(false, true);
#undef PRDC_LAUNCH
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
