// Latent-space tools (gfx950): the device side of contrad_amd/latent.py.
//
//   latent_pair      rows a, b fp32 [n][d], t fp32 [n], dt double -> the points of the path from a to b at t_i (out0) and at
//                    t_i + dt (out1, the sum formed in float64).  mode 0: lerp a + t (b - a).  mode 1: the slerp of Karras et
//                    al.: a^, b^ the normalised rows, c = normalize(b^ - (a^.b^) a^), theta = atan2(|b^ - (a^.b^) a^|, a^.b^)
//                    (no acos: near a^.b^ = 1 its derivative is unbounded), point = normalize(a^ cos(t theta) + c sin(t theta)).
//                    One wave owns one row and walks it in strides of 64; the five row sums (|a|^2, |b|^2, a^.b^, |c|^2 and the
//                    point's |.|^2) are wave reductions in float64, so every lane holds the same intermediates and both points
//                    of a row come from one set of them.  All arithmetic is float64, one rounding to fp32 at the store.  The
//                    rows are read again from L1/L2 in each pass: d is free, and 512 floats per row do not leave L1.
//                    Degenerate rows: when |b^ - (a^.b^) a^| is 0 to rounding -- not above (d + 16) 2^-52, the float64 chain
//                    of the dot product, below which the direction of c is rounding noise -- the point is a^ for every t
//                    (b = a, b = -a).  x / max(|x|, 1e-300) sends a zero row to zero.
//   latent_styles    out[b][l][:] = w_avg + psi[l] (src - w_avg), src = w[b] if l < cross[b] else w2[b], in fp32; one thread per
//                    element.  A layer with psi[l] == 1, and every layer when psi is null, stores the source row's bits.
//   pair_dist        out[i] = scale |A^_i - B^_i|^2 in float64, x^ = x / max(|x|, 1e-12): the difference is taken first, so two
//                    rows 1e-4 apart keep every digit that the similarity form 2 - 2 s cancels.  One workgroup of 256 owns one
//                    pair: pass 1 adds the two squared norms, pass 2 the squared differences of the quotients.  Up to
//                    d = PAIR_RESIDENT_D the fp32 rows wait in LDS between the passes (each is read from HBM once); above, pass
//                    2 reads them again.  Sums: per thread in index order with stride 256, then a float64 wave butterfly, then
//                    the four wave sums in order.
// Every buffer is an output with one owner per element: no scratch, no atomics, two calls are bitwise equal.
#include "../../../include/contrad_hip.h"
#include "../common.h"

#include <stdint.h>

namespace {

constexpr int PAIR_THREADS = 256;
// Two fp32 rows of 16384 are 128 KiB of the CU's 160 KiB LDS: the largest power of two that fits beside the reduction's
// 64 bytes.  SNDCGAN's 8192 takes 64 KiB, so two workgroups share a CU there.
constexpr int PAIR_RESIDENT_D = 16384;
constexpr double PAIR_TINY = 1e-12;
constexpr double LATENT_TINY = 1e-300;
constexpr int STYLES_THREADS = 256;

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The sum over the workgroup of PAIR_THREADS, the same value in every thread.  red holds 4 doubles; ends with a barrier
// so that red may be used again.
__device__ __forceinline__ double block_sum64(double v, double* red) {
  v = wave_sum64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__global__ void __launch_bounds__(64) latent_pair_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         const float* __restrict__ t, double dt, int mode,
                                                         float* __restrict__ out0, float* __restrict__ out1, int d) {
  const long long row = blockIdx.x;
  const int lane = threadIdx.x;
  const float* ar = a + row * d;
  const float* br = b + row * d;
  float* o0 = out0 + row * d;
  float* o1 = out1 + row * d;
  const double t0 = (double)t[row];
  const double tt[2] = {t0, t0 + dt};
  if (mode == 0) {
    for (int j = lane; j < d; j += 64) {
      const double x = (double)ar[j], y = (double)br[j] - x;
      o0[j] = (float)(x + tt[0] * y);
      o1[j] = (float)(x + tt[1] * y);
    }
    return;
  }
  double sa = 0.0, sb = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double x = (double)ar[j], y = (double)br[j];
    sa += x * x;
    sb += y * y;
  }
  const double na = fmax(sqrt(wave_sum64(sa)), LATENT_TINY), nb = fmax(sqrt(wave_sum64(sb)), LATENT_TINY);
  double sd = 0.0;
  for (int j = lane; j < d; j += 64) sd += ((double)ar[j] / na) * ((double)br[j] / nb);
  const double dot = wave_sum64(sd);
  double sc = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double x = (double)ar[j] / na, c = (double)br[j] / nb - dot * x;
    sc += c * c;
  }
  const double nc = sqrt(wave_sum64(sc));
  if (!(nc > (double)(d + 16) * 0x1p-52)) {                           // b^ = +-a^ to rounding: the path is the point a^
    for (int j = lane; j < d; j += 64) o0[j] = o1[j] = (float)((double)ar[j] / na);
    return;
  }
  const double theta = atan2(nc, dot);
  for (int e = 0; e < 2; ++e) {
    double sn, cs;
    sincos(tt[e] * theta, &sn, &cs);
    double sp = 0.0;
    for (int j = lane; j < d; j += 64) {
      const double x = (double)ar[j] / na, c = ((double)br[j] / nb - dot * x) / nc;
      const double p = x * cs + c * sn;
      sp += p * p;
    }
    const double np = fmax(sqrt(wave_sum64(sp)), LATENT_TINY);
    float* o = e ? o1 : o0;
    for (int j = lane; j < d; j += 64) {
      const double x = (double)ar[j] / na, c = ((double)br[j] / nb - dot * x) / nc;
      o[j] = (float)((x * cs + c * sn) / np);
    }
  }
}

__global__ void __launch_bounds__(STYLES_THREADS) latent_styles_kernel(const float* __restrict__ w, const float* __restrict__ w2,
                                                                       const float* __restrict__ w_avg,
                                                                       const float* __restrict__ psi,
                                                                       const float* __restrict__ cross,
                                                                       float* __restrict__ out, long long total, int L, int d) {
  const long long g = (long long)blockIdx.x * STYLES_THREADS + threadIdx.x;
  if (g >= total) return;
  const int j = (int)(g % d);
  const long long bl = g / d;
  const int l = (int)(bl % L);
  const long long bi = bl / L;
  const float* src = (cross && !((float)l < cross[bi])) ? w2 : w;
  const float s = src[bi * d + j];
  float r = s;
  if (psi) {
    const float p = psi[l];
    if (p != 1.0f) {
      const float m = w_avg[j];
      r = m + p * (s - m);
    }
  }
  out[g] = r;
}

template <bool RESIDENT>
__global__ void __launch_bounds__(PAIR_THREADS) pair_dist_kernel(const float* __restrict__ A, long long ldA,
                                                                 const float* __restrict__ B, long long ldB, int d, double scale,
                                                                 double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rows[];        // RESIDENT: [2][d] behind the 4 doubles of the reduction
  double* red = reinterpret_cast<double*>(rows);
  float* la = rows + 8;
  float* lb = la + d;
  const float* ar = A + (long long)blockIdx.x * ldA;
  const float* br = B + (long long)blockIdx.x * ldB;
  double sa = 0.0, sb = 0.0;
  for (int j = threadIdx.x; j < d; j += PAIR_THREADS) {
    const float xf = ar[j], yf = br[j];
    if (RESIDENT) {
      la[j] = xf;                                                      // (read back by the thread that wrote it: no barrier)
      lb[j] = yf;
    }
    const double x = (double)xf, y = (double)yf;
    sa += x * x;
    sb += y * y;
  }
  const double na = fmax(sqrt(block_sum64(sa, red)), PAIR_TINY), nb = fmax(sqrt(block_sum64(sb, red)), PAIR_TINY);
  double acc = 0.0;
  for (int j = threadIdx.x; j < d; j += PAIR_THREADS) {
    const double x = (double)(RESIDENT ? la[j] : ar[j]), y = (double)(RESIDENT ? lb[j] : br[j]);
    const double df = x / na - y / nb;
    acc += df * df;
  }
  acc = block_sum64(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = scale * acc;
}

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

constexpr size_t PAIR_RED_BYTES = 4 * sizeof(double);

}  // namespace

extern "C" int contrad_latent_pair(const float* a, const float* b, const float* t, double dt, int mode, float* out0, float* out1,
                                   long long n, int d, contrad_stream_t stream) {
  CONTRAD_ARG(a && b && t && out0 && out1);
  CONTRAD_ARG(mode == 0 || mode == 1);
  CONTRAD_ARG(n >= 1 && n <= 0x7fffffffll && d >= 1);
  CONTRAD_ARG(dt == dt && dt - dt == 0.0);                            // finite
  CONTRAD_ARG(out0 != out1);
  hipLaunchKernelGGL(latent_pair_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, a, b, t, dt, mode, out0, out1, d);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_latent_styles(const float* w, const float* w2, const float* w_avg, const float* psi, const float* cross,
                                     float* out, int B, int L, int d, contrad_stream_t stream) {
  CONTRAD_ARG(w && out);
  CONTRAD_ARG(B >= 1 && L >= 1 && d >= 1);
  CONTRAD_ARG((w2 == nullptr) == (cross == nullptr));
  CONTRAD_ARG((w_avg == nullptr) == (psi == nullptr));
  const long long total = (long long)B * L * d;
  CONTRAD_ARG(cdivll(total, STYLES_THREADS) <= 0x7fffffffll);
  hipLaunchKernelGGL(latent_styles_kernel, dim3((unsigned)cdivll(total, STYLES_THREADS)), dim3(STYLES_THREADS), 0,
                     (hipStream_t)stream, w, w2, w_avg, psi, cross, out, total, L, d);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_pair_dist_resident_d(void) { return PAIR_RESIDENT_D; }

extern "C" int contrad_pair_dist(const float* A, long long ldA, const float* B, long long ldB, long long n, int d, double scale,
                                 double* out, contrad_stream_t stream) {
  CONTRAD_ARG(A && B && out);
  CONTRAD_ARG(n >= 1 && n <= 0x7fffffffll && d >= 1 && ldA >= d && ldB >= d);
  CONTRAD_ARG(((uintptr_t)out & 7) == 0);
  CONTRAD_ARG(scale == scale && scale - scale == 0.0);                // finite
  hipStream_t st = (hipStream_t)stream;
  if (d <= PAIR_RESIDENT_D) {
    const size_t lds = PAIR_RED_BYTES + 2 * (size_t)d * sizeof(float);
    static bool done[64] = {};
    const int rc = allow_lds(reinterpret_cast<const void*>(&pair_dist_kernel<true>),
                             PAIR_RED_BYTES + 2 * (size_t)PAIR_RESIDENT_D * sizeof(float), done);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(pair_dist_kernel<true>, dim3((unsigned)n), dim3(PAIR_THREADS), lds, st, A, ldA, B, ldB, d, scale, out);
  } else {
    hipLaunchKernelGGL(pair_dist_kernel<false>, dim3((unsigned)n), dim3(PAIR_THREADS), PAIR_RED_BYTES, st, A, ldA, B, ldB, d, scale,
                       out);
  }
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
