// Weighted k-nearest-neighbour vote on a similarity matrix (gfx950): per query row the top k columns, their class
// vote and the predicted class, in ONE launch, one 256-thread workgroup per row.  No float atomics; every output
// element is written once and every float sum has a fixed order, so two calls are bitwise equal.
//
// The key order (NaN lowest, -0.0 == +0.0, ties by ascending column), the radix select of the k-th largest key and the
// round scan of the ordered pass are csrc/simrow.h's, shared with prdc.hip.  This file owns what follows the threshold key:
//
//   compact   a neighbour is ranked by the 64-bit word (key << 32 | ~column) descending.  One ordered pass over the row
//             (a thread takes 4 consecutive columns, one scan numbers both tallies, packed into one word): every column
//             above the threshold key and, in column order, the first k - count columns equal to it.
//   sort      bitonic sort of the (at most 1024, padded to a power of two) 64-bit words in LDS.
//   vote      idx / val out (val re-read from S: the very floats); labels and expf(val * inv_temp) staged in LDS;
//             thread c adds the weights of class c in rank order; the block's argmax under the same key order.
//
// Leave-self-out (contrad_knn_select_loo): with self0 >= 0 row q of the launch is row self0 + q of the bank it is compared
// with and leaves that column out BY INDEX (contrad_prdc_kth's convention; a duplicate elsewhere in the bank is a neighbour
// like any other).  A run-time, block-uniform argument of the one kernel: the column takes part in no histogram and in
// neither tally of the compaction, so every step sees a row of n - 1 columns.  self0 < 0 is the kernel as it was.
//
// The row is read five times (four digits and the compaction) and never staged: the caller hands over chunks of S small
// enough to be served from cache (contrad_amd/knn.py), and at n = 50 000 a row is 200 KB, beyond the LDS of a CU.
#include "../../include/contrad_hip.h"
#include "simrow.h"
#include <type_traits>

namespace {

constexpr int KNN_THREADS = simrow::THREADS;
constexpr int KNN_MAX_K = 1024;
constexpr int KNN_MAX_C = 1024;

__device__ __forceinline__ unsigned long long knn_word(unsigned key, unsigned col) {
  return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - col);
}

__global__ __launch_bounds__(KNN_THREADS) void knn_select_kernel(const float* __restrict__ S, long long ldS, int n,
                                                                 long long self0, const long long* __restrict__ labels,
                                                                 int C, int k, int P, float inv_temp,
                                                                 int* __restrict__ idx, float* __restrict__ val,
                                                                 float* __restrict__ scores, int* __restrict__ pred) {
  __shared__ unsigned hist[4][256];
  __shared__ unsigned long long words[KNN_MAX_K];
  __shared__ int lab_s[KNN_MAX_K];
  __shared__ float w_s[KNN_MAX_K];
  __shared__ unsigned wtot[2][4];
  __shared__ unsigned sel[2];
  __shared__ unsigned long long best[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long q = blockIdx.x;
  const float* __restrict__ row = S + q * ldS;
  const unsigned un = (unsigned)n;
  // Leave-self-out (block-uniform): row q of the launch is global row self0 + q and never sees column `ex` of its own bank,
  // whatever that column holds.  Select and compaction are written once and compiled twice: LOO = false is the row as it
  // ever was, without a test per element; LOO = true skips `ex` in every histogram and in both tallies of the compaction.
  const bool loo_row = self0 >= 0 && self0 + q < (long long)n;
  const unsigned ex = loo_row ? (unsigned)(self0 + q) : 0xffffffffu;
  unsigned T = 0u, cgt = 0u, krem = (unsigned)k;

  auto select_and_compact = [&](auto loo) {
    constexpr bool LOO = decltype(loo)::value;
    // ---- the k-th largest key T; `krem` of the columns equal to it are neighbours ----
    T = simrow::kth_key<LOO, 4, 1>(row, un, ex, hist, wtot, sel, krem);
    cgt = (unsigned)k - krem;                                                           // cgt columns have a key above T

    // ---- ordered compaction: words[0, cgt) keys above T, words[cgt, k) the first krem columns equal to T ----
    for (int r = k + tid; r < P; r += KNN_THREADS) words[r] = 0ull;                     // padding sorts last
    unsigned base_g = 0u, base_e = 0u;
    int buf = 0;
    for (unsigned c0 = 0u; c0 < un; c0 += simrow::CHUNK, buf ^= 1) {
      const unsigned j0 = c0 + 4u * tid;
      unsigned key4[4];
      unsigned g = 0u, e = 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool in = j0 + i < un && !(LOO && j0 + i == ex);   // the column left out is in neither tally
        key4[i] = in ? simrow::key(row[j0 + i]) : 0u;
        g += (in && key4[i] > T) ? 1u : 0u;
        e += (in && key4[i] == T) ? 1u : 0u;
      }
      const unsigned p = g | (e << 16);                  // both counts <= 1024 per round: the two scans share a word
      unsigned tot;
      const unsigned off = simrow::round_scan(p, wtot[buf], tot);
      unsigned pg = base_g + (off & 0xffffu), pe = base_e + (off >> 16);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (j0 + i >= un) break;
        if (LOO && j0 + i == ex) continue;               // never written (its key4 is 0, which a NaN threshold T equals)
        if (key4[i] > T) {
          words[pg++] = knn_word(key4[i], j0 + i);       // pg < cgt: exactly cgt columns lie above T
        } else if (key4[i] == T) {
          if (pe < krem) words[cgt + pe] = knn_word(key4[i], j0 + i);
          ++pe;
        }
      }
      base_g += tot & 0xffffu;
      base_e += tot >> 16;
      if (base_g >= cgt && base_e >= krem) break;        // (uniform) the k neighbours are complete: `ex` is in no count
    }
  };
  if (loo_row) select_and_compact(std::true_type{});
  else select_and_compact(std::false_type{});

  // ---- bitonic sort, descending ----
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (P >> 1); t += KNN_THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool desc = (i & size) == 0;
        const unsigned long long a = words[i], b = words[j];
        if ((a < b) == desc) {
          words[i] = b;
          words[j] = a;
        }
      }
    }
  }
  __syncthreads();

  // ---- outputs and the vote ----
  for (int r = tid; r < k; r += KNN_THREADS) {
    unsigned j = 0xffffffffu - (unsigned)(words[r] & 0xffffffffull);
    j = j < un ? j : un - 1u;                          // (always j < n; keeps every read inside the row regardless)
    const float v = row[j];
    idx[q * k + r] = (int)j;
    val[q * k + r] = v;
    const long long l = labels[j];
    lab_s[r] = (l >= 0 && l < C) ? (int)l : -1;        // a label outside [0, C) votes for nobody
    w_s[r] = expf(v * inv_temp);
  }
  __syncthreads();
  unsigned long long mine = 0ull;
  for (int c = tid; c < C; c += KNN_THREADS) {
    float s = 0.f;
    for (int r = 0; r < k; ++r)
      if (lab_s[r] == c) s += w_s[r];
    scores[q * C + c] = s;
    const unsigned long long cand = knn_word(simrow::key(s), (unsigned)c);
    mine = cand > mine ? cand : mine;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(mine, o, 64);
    mine = t > mine ? t : mine;
  }
  if (lane == 0) best[w] = mine;
  __syncthreads();
  if (tid == 0) {
    unsigned long long m = best[0];
    for (int ww = 1; ww < 4; ++ww) m = best[ww] > m ? best[ww] : m;
    pred[q] = (int)(0xffffffffu - (unsigned)(m & 0xffffffffull));
  }
}

inline bool knn_shape_ok(int M, int n, int k, int C) {
  return M >= 1 && n >= 1 && k >= 1 && k <= n && k <= KNN_MAX_K && C >= 1 && C <= KNN_MAX_C;
}

// The one launcher.  With 0 <= self0 < n the shortest row keeps n - 1 columns: k <= n - 1, or the radix select would look
// for a k-th place among fewer than k candidates.
int knn_launch(const float* S, long long ldS, int M, int n, long long self0, const long long* labels, int C, int k,
               float inv_temp, int* idx, float* val, float* scores, int* pred, void* workspace, long long workspace_bytes,
               contrad_stream_t stream) {
  CONTRAD_ARG(S && labels && idx && val && scores && pred);
  CONTRAD_ARG(knn_shape_ok(M, n, k, C) && ldS >= n);
  CONTRAD_ARG(!(self0 >= 0 && self0 < n) || k <= n - 1);
  const long long need = contrad_knn_select_workspace_bytes(M, n, k, C);
  CONTRAD_ARG(workspace_bytes >= need && (need == 0 || workspace != nullptr));
  int P = 1;
  while (P < k) P <<= 1;
  hipLaunchKernelGGL(knn_select_kernel, dim3(M), dim3(KNN_THREADS), 0, (hipStream_t)stream, S, ldS, n, self0, labels, C, k,
                     P, inv_temp, idx, val, scores, pred);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" long long contrad_knn_select_workspace_bytes(int M, int n, int k, int C) {
  if (!knn_shape_ok(M, n, k, C)) return -22;
  return 0;                                            // this form keeps everything in LDS
}

extern "C" int contrad_knn_select(const float* S, long long ldS, int M, int n, const long long* labels, int C, int k,
                                  float inv_temp, int* idx, float* val, float* scores, int* pred, void* workspace,
                                  long long workspace_bytes, contrad_stream_t stream) {
  return knn_launch(S, ldS, M, n, -1, labels, C, k, inv_temp, idx, val, scores, pred, workspace, workspace_bytes, stream);
}

extern "C" int contrad_knn_select_loo(const float* S, long long ldS, int M, int n, long long self0, const long long* labels,
                                      int C, int k, float inv_temp, int* idx, float* val, float* scores, int* pred,
                                      void* workspace, long long workspace_bytes, contrad_stream_t stream) {
  return knn_launch(S, ldS, M, n, self0, labels, C, k, inv_temp, idx, val, scores, pred, workspace, workspace_bytes, stream);
}
