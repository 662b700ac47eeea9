// What the kernels that read a similarity matrix S = Q bank^T share (gfx950): knn.hip, prdc.hip and kid.hip.  Each piece
// exists here once; every caller is a 256-thread workgroup (four waves of 64) and declares the LDS arrays it hands over
// itself.
//
//   key          the order of a row, stated once: a float becomes a 32-bit key whose unsigned order is NaN below every
//                number (NaN -> 0; the key of -inf is 0x007fffff), -0.0 equal to +0.0, then the usual sign flip.  Columns
//                with equal keys rank by ascending column: the k-th place among them is found in column order.
//   kth_key      the k-th largest key of a row by radix select, four 8-bit digits from the top: per digit an LDS histogram
//                (one per wave, integer adds: the counts do not depend on the order of arrival) of the columns that match
//                the digits fixed so far, a suffix sum over the 256 bins, the bin that holds the k-th place.  The row is
//                read once per digit.  EXCL leaves column `ex` out of every histogram BY INDEX, whatever it holds
//                (leave-self-out; EXCL = false compiles no test per element).  DIGITS and COLUMNS are the unroll counts
//                of the digit loop and of the histogram loop, each caller's own, because this launch moves by percents
//                on one instruction per element (profiles/nearest.txt): knn 4, 1; prdc 1, 4 (profiles/simrow.txt).
//   round_scan   one round of an ordered pass over the row (4 x 256 columns, a thread takes four consecutive ones): the
//                wave's inclusive scan of a thread's packed count, the four wave totals in wtot[buf] (double-buffered:
//                one __syncthreads() per round), the exclusive offset of the thread in the block and the round's total.
//   load_tile    the row-tile walk: a workgroup takes 4 * rpw rows x 256 columns, a wave every fourth row (r0, r0 + 4,
//                ...), a lane four consecutive columns from c0 (one 16-byte load where the address allows), four rows in
//                flight; a round's missing rows re-read the wave's last one.  A column outside [0, n) reads as `fill`.
//                The row index keeps the caller's type R (kid's is long long: S may be larger than 2^31 elements);
//                per_row(u, i) is called with row u's index i behind its load.
#pragma once
#include "common.h"

namespace simrow {

constexpr int THREADS = 256;
constexpr unsigned CHUNK = 4 * THREADS;             // columns per round of an ordered pass
constexpr int COLS = 256;                           // columns of a row tile: 4 per lane

__device__ __forceinline__ unsigned key(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Returns the k-th largest key for k = krem on entry; on return it is the krem-th of the columns equal to it.
template <bool EXCL, int DIGITS, int COLUMNS>
__device__ __forceinline__ unsigned kth_key(const float* row, unsigned un, unsigned ex, unsigned (&hist)[4][256],
                                            unsigned (&wtot)[2][4], unsigned (&sel)[2], unsigned& krem) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned prefix = 0u;
#pragma unroll DIGITS
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int i = tid; i < 4 * 256; i += THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();
#pragma unroll COLUMNS
    for (unsigned j = tid; j < un; j += THREADS) {
      const unsigned kj = key(row[j]);
      if (!(EXCL && j == ex) && (kj & himask) == prefix) atomicAdd(&hist[w][(kj >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned cnt = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];   // thread t owns bin t
    unsigned suf = cnt;                                                               // sum over the bins >= t of this wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_down(suf, o, 64);
      if (lane + o < 64) suf += t;
    }
    if (lane == 0) wtot[0][w] = suf;
    __syncthreads();
    unsigned above = suf - cnt;                                                       // columns in higher bins
    for (int ww = w + 1; ww < 4; ++ww) above += wtot[0][ww];
    if (above < krem && krem <= above + cnt) {                                        // exactly one bin
      sel[0] = (unsigned)tid;
      sel[1] = krem - above;
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    krem = sel[1];
  }
  return prefix;
}

// p: this thread's count(s) of the round, packed so that no field of the block's sum overflows.  Returns the sum over the
// threads before this one; tot: over the block.
__device__ __forceinline__ unsigned round_scan(unsigned p, unsigned (&wt)[4], unsigned& tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = p;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wt[w] = inc;
  __syncthreads();
  unsigned off = inc - p;
  tot = 0u;
  for (int ww = 0; ww < 4; ++ww) {
    const unsigned t = wt[ww];
    if (ww < w) off += t;
    tot += t;
  }
  return off;
}

template <typename R, typename F>
__device__ __forceinline__ void load_tile(float (&v)[4][4], const float* S, long long ldS, R r0, int t0, int rows,
                                          long long c0, int n, int vec_ok, float fill, F per_row) {
  const bool whole = vec_ok && c0 + 3 < n;             // vec_ok: the host found ldS % 4 == 0 and S 16-byte aligned
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long i = r0 + 4 * min(t0 + u, rows - 1);
    const float* __restrict__ row = S + i * ldS;
    if (whole) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(row + c0);
      v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[u][j] = c0 + j < n ? row[c0 + j] : fill;
    }
    per_row(u, i);
  }
}

}  // namespace simrow
