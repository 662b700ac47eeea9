// Softmax-regression head for linear evaluation (gfx950): logits, cross-entropy + top-k meters, weight gradient
// fused with the SGD update.  Three launches per training iteration, two per evaluation iteration, no host
// synchronisation and no float atomics: every sum has a fixed order, so results are bitwise repeatable.
//
//   1. linhead_logits_kernel<CT>   partial[S][N][C]: block = 64 rows x one K-slice, 256 threads as 16 row groups x
//      16 class groups, 4 rows x CT classes per thread (CT = ceil(C / 16) <= 8), F and W staged through LDS in
//      64-wide K chunks and read back as 16-byte vectors along K.
//   2. linhead_loss_kernel         one block per sample: its four waves sum the S partials in a fixed order, one wave adds
//      the bias and does log-sum-exp, cross-entropy, top-1 / top-5 by the strictly-greater rule and dlogits; the row's
//      loss and hits go to a scratch word and the block that arrives last adds their fixed-order float64 sums to meters[4].
//   3. linhead_wgrad_kernel<CT>    block = 32 K columns x all classes, 8 k-quads x 32 class groups, 4 k x CT classes
//      per thread (CT = ceil(C / 32) <= 4), F and dlogits staged through LDS 64 rows at a time, rows summed in order;
//      the epilogue writes gradW and / or W -= lr * gradW with lr read from device memory.
//
// Plain v_fma_f32 instead of the fp32 MFMAs: the head is a skinny product (C <= 128, 0.04 - 0.4 GFLOP against 8 MB of
// features); with C = 10 a 16-wide MFMA tile would be 3/8 padding and the arithmetic is a few microseconds either
// way, so the launches are bound by launch latency and by streaming F once, not by the multiply rate.  FMAs keep
// one code path for every C and K (no padded-operand layouts) and an exact fp32 accumulation order that is easy to state.
#include "../../include/contrad_hip.h"
#include "common.h"

namespace {

constexpr int LH_TM = 64;       // rows per block, kernel 1
constexpr int LH_KC = 64;       // K chunk staged in LDS, kernel 1
constexpr int LH_LD = LH_KC + 4;  // LDS row stride in floats: one 16-byte slot of padding
constexpr int LH_KT = 32;       // K columns per block, kernel 3
constexpr int LH_NT = 64;       // rows staged per round, kernel 3
constexpr int LH_WS_HEAD = 64;  // floats in front of the workspace: the arrival counter on a line of its own

struct LinheadPlan {
  int S;         // K-splits of launch 1
  int cps;       // 64-wide K chunks per split
  int ct;        // classes per thread of launch 1
  int ct3;       // classes per thread of launch 3
  int row_tiles; // 64-row tiles of launch 1
};

// Pure function of (N, K, C): about two blocks per CU over the row tiles, but never more splits than keep the partial
// sums (S * N * C floats) below the features themselves (N * K floats).
LinheadPlan linhead_plan(int N, int K, int C) {
  LinheadPlan p;
  p.ct = cdiv(C, 16);
  p.ct3 = cdiv(C, 32);
  p.row_tiles = cdiv(N, LH_TM);
  const int nchunks = cdiv(K, LH_KC);
  int want = cdiv(512, p.row_tiles);
  const int cap = K / (16 * p.ct) > 1 ? K / (16 * p.ct) : 1;
  if (want > cap) want = cap;
  if (want > nchunks) want = nchunks;
  p.cps = cdiv(nchunks, want);
  p.S = cdiv(nchunks, p.cps);
  return p;
}

__device__ __forceinline__ void fma4(float& acc, const float4 a, const float4 b) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  acc = fmaf(a.w, b.w, acc);
}

// Stage rows [r0, r0 + nrows) x columns [k0, k0 + LH_KC) of a row-major matrix (row stride ld, `rows` x `K` valid) into
// tile[nrows][LH_LD], zero outside.  vec: 16-byte loads are legal (base 16-byte aligned, ld % 4 == 0).
__device__ __forceinline__ void stage_tile(float* tile, const float* __restrict__ M, long long ld, int rows, int K,
                                           int r0, int nrows, int k0, bool vec) {
  for (int i = threadIdx.x; i < nrows * (LH_KC / 4); i += blockDim.x) {
    const int r = i / (LH_KC / 4), q = i % (LH_KC / 4);
    const int k = k0 + q * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < rows) {
      const float* src = M + (long long)(r0 + r) * ld + k;
      if (vec && k + 3 < K) {
        v = *reinterpret_cast<const float4*>(src);
      } else {
        if (k < K) v.x = src[0];
        if (k + 1 < K) v.y = src[1];
        if (k + 2 < K) v.z = src[2];
        if (k + 3 < K) v.w = src[3];
      }
    }
    *reinterpret_cast<float4*>(tile + r * LH_LD + q * 4) = v;
  }
}

template <int CT>
__global__ __launch_bounds__(256) void linhead_logits_kernel(const float* __restrict__ F, int ldf,
                                                             const float* __restrict__ W, int N, int K, int C, int S,
                                                             int cps, int row_tiles, int fvec, int wvec,
                                                             float* __restrict__ partial, unsigned* counter) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* fs = reinterpret_cast<float*>(smem);        // [LH_TM][LH_LD]
  float* wsm = fs + LH_TM * LH_LD;                   // [16 * CT][LH_LD]
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter = 0u;   // arrival counter of launch 2 (a kernel boundary later)
  const int s = blockIdx.x / row_tiles, rt = blockIdx.x % row_tiles;
  const int r0 = rt * LH_TM;
  const int rg = threadIdx.x >> 4, cg = threadIdx.x & 15;
  float acc[4][CT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = 0.f;
  const int chunk0 = s * cps;
  for (int ch = chunk0; ch < chunk0 + cps; ++ch) {
    const int k0 = ch * LH_KC;
    if (k0 >= K) break;
    __syncthreads();
    stage_tile(fs, F, ldf, N, K, r0, LH_TM, k0, fvec != 0);
    stage_tile(wsm, W, K, C, K, 0, 16 * CT, k0, wvec != 0);
    __syncthreads();
    // A chunk's 64 products are summed on their own and enter the split's sum as one term: with few K-splits (from about 2^16
    // rows on the plan has one) a single fp32 chain would run over all of K and lose about a decimal digit.  One chunk per split:
    // bitwise as before.  Costs 4 * CT registers; the kernel's time with them has not been measured.
    float cacc[4][CT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j) cacc[i][j] = 0.f;
#pragma unroll 4
    for (int q = 0; q < LH_KC / 4; ++q) {
      float4 a[4], b[CT];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const float4*>(fs + (rg * 4 + i) * LH_LD + q * 4);
#pragma unroll
      for (int j = 0; j < CT; ++j) b[j] = *reinterpret_cast<const float4*>(wsm + (cg + 16 * j) * LH_LD + q * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) fma4(cacc[i][j], a[i], b[j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j) acc[i][j] += cacc[i][j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + rg * 4 + i;
    if (r >= N) continue;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int c = cg + 16 * j;
      if (c < C) partial[((long long)s * N + r) * C + c] = acc[i][j];
    }
  }
}

// One block per row.  The 4 x 128 lane slots of the block (4 waves x 64 lanes x 2) are split into 4 * G groups of
// CW = 16 / 32 / 64 / 128 >= C classes (G = 128 / CW): group q adds the partial sums s = q, q + 4G, ... in order (16
// loads in flight at a time), then wave 0 adds the 4G group sums in order and does the row's softmax arithmetic.
// rows[n] = {loss bits, top-1 hit | top-5 hit << 1} in ONE 8-byte word.
__global__ __launch_bounds__(256) void linhead_loss_kernel(const float* __restrict__ partial,
                                                           const float* __restrict__ bias,
                                                           const long long* __restrict__ y, int N, int C, int S,
                                                           float dl_scale, float* __restrict__ logits,
                                                           float* __restrict__ dlogits, double* meters,
                                                           unsigned long long* rows, unsigned* counter) {
  __shared__ double red[4 * 3 + 1];
  __shared__ float grp[4][128];
  __shared__ unsigned last;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.x;                          // < N: the grid is N blocks
  const int CW = C <= 16 ? 16 : C <= 32 ? 32 : C <= 64 ? 64 : 128;
  const int G = 128 / CW;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int slot = lane + 64 * h;
    const int c = slot % CW, q = w * G + slot / CW;
    float v = 0.f;
    if (c < C) {
      const float* src = partial + (long long)n * C + c;
      const long long step = (long long)N * C;
      for (int s0 = q; s0 < S; s0 += 64 * G) {
        float t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int s = s0 + i * 4 * G;
          t[i] = (s < S) ? src[s * step] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) v += t[i];
      }
    }
    grp[w][slot] = v;
  }
  __syncthreads();
  if (w == 0) {
    float l[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      float v = -INFINITY;
      if (c < C) {
        v = 0.f;
        for (int ww = 0; ww < 4; ++ww)
          for (int g = 0; g < G; ++g) v += grp[ww][g * CW + c];
        if (bias) v += bias[c];
        if (logits) logits[(long long)n * C + c] = v;
      }
      l[h] = v;
    }
    if (y != nullptr) {
      const float m = wave_max(fmaxf(l[0], l[1]));
      const float e0 = (lane < C) ? expf(l[0] - m) : 0.f;
      const float e1 = (lane + 64 < C) ? expf(l[1] - m) : 0.f;
      const float se = wave_sum(e0 + e1);
      const float lse = m + logf(se);
      const long long lab = y[n];
      const bool ok = lab >= 0 && lab < C;
      const int labi = ok ? (int)lab : 0;                 // never indexes out of range
      const float mine = (labi < 64) ? l[0] : l[1];
      const float ly = __shfl(mine, labi & 63, 64);
      const float above = wave_sum(((lane < C && l[0] > ly) ? 1.f : 0.f) + ((lane + 64 < C && l[1] > ly) ? 1.f : 0.f));
      if (dlogits) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int c = lane + 64 * h;
          if (c < C) {
            const float p = expf(l[h] - lse);
            dlogits[(long long)n * C + c] = ok ? (p - (c == labi ? 1.f : 0.f)) * dl_scale : 0.f;
          }
        }
      }
      if (lane == 0 && meters != nullptr) {
        const unsigned hits = ok ? ((above < 1.f ? 1u : 0u) | (above < 5.f ? 2u : 0u)) : 0u;
        const unsigned long long word = ((unsigned long long)hits << 32) | __float_as_uint(ok ? lse - ly : 0.f);
        // write-through (agent-scope) store of the one word another block will read: no release fence needed
        __hip_atomic_store(rows + n, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (t == gridDim.x - 1) ? 1u : 0u;
        if (t == gridDim.x - 1) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      }
    }
  }
  if (y == nullptr || meters == nullptr) return;           // (uniform over the grid)
  // Last-block-done reduction of the per-row words: the storing lane drains its write-through store and takes a ticket;
  // the block that draws the last ticket acquires and sums every row in a fixed order (agent-scope loads).
  __syncthreads();
  if (!last) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) {
    const unsigned long long r = __hip_atomic_load(rows + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a0 += (double)__uint_as_float((unsigned)r);
    a1 += (double)((r >> 32) & 1u);
    a2 += (double)((r >> 33) & 1u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o, 64); a1 += __shfl_xor(a1, o, 64); a2 += __shfl_xor(a2, o, 64);
  }
  if (lane == 0) { red[w * 3] = a0; red[w * 3 + 1] = a1; red[w * 3 + 2] = a2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    meters[0] += ((red[0] + red[3]) + red[6]) + red[9];
    meters[1] += ((red[1] + red[4]) + red[7]) + red[10];
    meters[2] += ((red[2] + red[5]) + red[8]) + red[11];
    meters[3] += (double)N;
    *counter = 0u;
  }
}

template <int CT>
__global__ __launch_bounds__(256) void linhead_wgrad_kernel(const float* __restrict__ F, int ldf,
                                                            const float* __restrict__ dl, int N, int K, int C,
                                                            int fvec, int wvec, const float* __restrict__ lr_dev,
                                                            float* W, float* b, float* gradW, float* gradb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CP = 32 * CT;
  float* fs = reinterpret_cast<float*>(smem);        // [LH_NT][LH_KT]
  float* ds = fs + LH_NT * LH_KT;                    // [LH_NT][CP]
  const int k0 = blockIdx.x * LH_KT;
  const int kq = threadIdx.x & 7, cg = threadIdx.x >> 3;
  float acc[CT][4];
  float bs[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    bs[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
  }
  // per round a thread stages two 16-byte pieces of F (64 rows x 8 quads = 512 pieces) and CP / 4 values of dlogits;
  // the next round's pieces are fetched into registers while this round is multiplied
  constexpr int DPT = LH_NT * CP / 256;
  const int fr = threadIdx.x >> 3, fq = threadIdx.x & 7;
  float4 fnext[2];
  float dnext[DPT];
  auto fetch = [&](int n0) {
    const int k = k0 + fq * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = n0 + fr + 32 * h;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < N) {
        const float* src = F + (long long)r * ldf + k;
        if (fvec && k + 3 < K) {
          v = *reinterpret_cast<const float4*>(src);
        } else {
          if (k < K) v.x = src[0];
          if (k + 1 < K) v.y = src[1];
          if (k + 2 < K) v.z = src[2];
          if (k + 3 < K) v.w = src[3];
        }
      }
      fnext[h] = v;
    }
#pragma unroll
    for (int i = 0; i < DPT; ++i) {
      const int e = threadIdx.x + 256 * i;
      const int r = e / CP, c = e % CP;
      dnext[i] = (n0 + r < N && c < C) ? dl[(long long)(n0 + r) * C + c] : 0.f;
    }
  };
  fetch(0);
  for (int n0 = 0; n0 < N; n0 += LH_NT) {
    __syncthreads();
    *reinterpret_cast<float4*>(fs + fr * LH_KT + fq * 4) = fnext[0];
    *reinterpret_cast<float4*>(fs + (fr + 32) * LH_KT + fq * 4) = fnext[1];
#pragma unroll
    for (int i = 0; i < DPT; ++i) ds[threadIdx.x + 256 * i] = dnext[i];
    __syncthreads();
    if (n0 + LH_NT < N) fetch(n0 + LH_NT);
#pragma unroll 8
    for (int r = 0; r < LH_NT; ++r) {
      const float4 f = *reinterpret_cast<const float4*>(fs + r * LH_KT + kq * 4);
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const float d = ds[r * CP + cg * CT + j];
        acc[j][0] = fmaf(d, f.x, acc[j][0]);
        acc[j][1] = fmaf(d, f.y, acc[j][1]);
        acc[j][2] = fmaf(d, f.z, acc[j][2]);
        acc[j][3] = fmaf(d, f.w, acc[j][3]);
        bs[j] += d;
      }
    }
  }
  const float lr = lr_dev ? *lr_dev : 0.f;
  const int k = k0 + kq * 4;
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    const int c = cg * CT + j;
    if (c >= C) continue;
    const long long o = (long long)c * K + k;
    if (wvec && k + 3 < K) {
      if (gradW) *reinterpret_cast<float4*>(gradW + o) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
      if (lr_dev) {
        float4 wv = *reinterpret_cast<float4*>(W + o);
        wv.x -= lr * acc[j][0]; wv.y -= lr * acc[j][1]; wv.z -= lr * acc[j][2]; wv.w -= lr * acc[j][3];
        *reinterpret_cast<float4*>(W + o) = wv;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (k + i >= K) break;
        if (gradW) gradW[o + i] = acc[j][i];
        if (lr_dev) W[o + i] -= lr * acc[j][i];
      }
    }
    if (blockIdx.x == 0 && kq == 0) {
      if (gradb) gradb[c] = bs[j];
      if (lr_dev && b) b[c] -= lr * bs[j];
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" long long contrad_linhead_workspace_bytes(int N, int K, int C) {
  if (N < 1 || K < 1 || C < 1 || C > 128) return -22;
  const LinheadPlan p = linhead_plan(N, K, C);
  return 4ll * (LH_WS_HEAD + 4ll * N + (long long)p.S * N * C);
}

extern "C" int contrad_linhead_plan(int N, int K, int C, int* splits, int* classes_per_thread, int* row_tiles) {
  CONTRAD_ARG(N >= 1 && K >= 1 && C >= 1 && C <= 128);
  const LinheadPlan p = linhead_plan(N, K, C);
  if (splits) *splits = p.S;
  if (classes_per_thread) *classes_per_thread = p.ct;
  if (row_tiles) *row_tiles = p.row_tiles;
  return 0;
}

extern "C" int contrad_linhead_fwd(const float* F, int ldf, const float* W, const float* b, const long long* y, int N,
                                   int K, int C, float dl_scale, float* logits, float* dlogits, double* meters4,
                                   void* ws, contrad_stream_t stream) {
  CONTRAD_ARG(F && W && ws && N >= 1 && K >= 1 && C >= 1 && C <= 128 && ldf >= K);
  CONTRAD_ARG(aligned16(ws));
  CONTRAD_ARG(y != nullptr || (dlogits == nullptr && meters4 == nullptr));
  const LinheadPlan p = linhead_plan(N, K, C);
  hipStream_t st = (hipStream_t)stream;
  unsigned* counter = reinterpret_cast<unsigned*>(ws);
  unsigned long long* rows = reinterpret_cast<unsigned long long*>(reinterpret_cast<float*>(ws) + LH_WS_HEAD);
  float* partial = reinterpret_cast<float*>(ws) + LH_WS_HEAD + 4ll * N;
  const int fvec = aligned16(F) && ldf % 4 == 0, wvec = aligned16(W) && K % 4 == 0;
  const int grid = p.S * p.row_tiles;
  const size_t lds = sizeof(float) * LH_LD * (LH_TM + 16 * p.ct);
#define LH_LOGITS(CT)                                                                                              \
  case CT:                                                                                                         \
    hipLaunchKernelGGL(linhead_logits_kernel<CT>, dim3(grid), dim3(256), lds, st, F, ldf, W, N, K, C, p.S, p.cps,  \
                       p.row_tiles, fvec, wvec, partial, counter);                                                 \
    break;
  switch (p.ct) {
    LH_LOGITS(1) LH_LOGITS(2) LH_LOGITS(3) LH_LOGITS(4) LH_LOGITS(5) LH_LOGITS(6) LH_LOGITS(7) LH_LOGITS(8)
    default: return -22;
  }
#undef LH_LOGITS
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(linhead_loss_kernel, dim3(N), dim3(256), 0, st, partial, b, y, N, C, p.S, dl_scale,
                     logits, dlogits, meters4, rows, counter);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_linhead_wgrad_sgd(const float* F, int ldf, const float* dlogits, int N, int K, int C,
                                         const float* lr_dev, float* W, float* b, float* gradW, float* gradb,
                                         contrad_stream_t stream) {
  CONTRAD_ARG(F && dlogits && N >= 1 && K >= 1 && C >= 1 && C <= 128 && ldf >= K);
  CONTRAD_ARG(lr_dev == nullptr || W != nullptr);
  CONTRAD_ARG(lr_dev != nullptr || gradW != nullptr || gradb != nullptr);
  const int ct3 = cdiv(C, 32);
  const int fvec = aligned16(F) && ldf % 4 == 0;
  const int wvec = K % 4 == 0 && (!gradW || aligned16(gradW)) && (!lr_dev || aligned16(W));
  hipStream_t st = (hipStream_t)stream;
  const int grid = cdiv(K, LH_KT);
  const size_t lds = sizeof(float) * LH_NT * (LH_KT + 32 * ct3);
#define LH_WGRAD(CT)                                                                                               \
  case CT:                                                                                                         \
    hipLaunchKernelGGL(linhead_wgrad_kernel<CT>, dim3(grid), dim3(256), lds, st, F, ldf, dlogits, N, K, C, fvec,   \
                       wvec, lr_dev, W, b, gradW, gradb);                                                          \
    break;
  switch (ct3) {
    LH_WGRAD(1) LH_WGRAD(2) LH_WGRAD(3) LH_WGRAD(4)
    default: return -22;
  }
#undef LH_WGRAD
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
