// Streaming kernels of conditional Langevin sampling in latent space (cDDLS, contrad_amd/cddls.py; gfx950): everything
// of one Langevin step that is not a convolution, plus the counter-based normal generator the step draws its noise from.
//
//   cddls_feature_seed_kernel      g = (g_head + c) * lrelu'(a6): the gradient entering D's trunk, from the logit head's
//                                  data gradient and the class row of the linear-evaluation head (one broadcast row);
//                                  two more index forms of the same arithmetic serve the residual D (snresnet18): the
//                                  pooled seed ((g[n][c] + c[c]) / T over the T pixels of the average pool) and the
//                                  residual join ((g_main + g_shortcut) * lrelu'(block input), two full tensors)
//   cddls_bn_relu_bwd_eval_kernel  dx = dy * [y > 0] * gamma / sqrt(running_var + eps): eval-mode BatchNorm + ReLU backward
//   cddls_compose_kernel           x = G(z) + eps * z2 (optionally clamped to [0, 1]: the final images)
//   cddls_image_end_kernel         gradient entering G's last transposed conv (through 0.5 tanh + 0.5) and the z2 update
//   cddls_latent_update_kernel     the z update with its clamp; the block that finishes last advances the step counter
//   cddls_energy_kernel            per-sample energy (diagnostic), one block per sample, fixed summation order
//   cddls_normal_fill_kernel       the generator alone (tests, the initial z2)
//
// Latent recovery (contrad_amd/recover.py) runs on the same chain with one more form of three of these kernels, each a
// loop of its own behind a wave-uniform launch argument (a null pointer selects the Langevin form, so those launches run
// the code they ran before):
//   cddls_energy_kernel, recovery form          pix[n] = |gout - x*|^2 / P, feat[n] = |phi - phi*|^2 / F, their weighted
//                                               sum, and the residual rows (2 lambda / F)(phi - phi*) the D backward seeds from
//   cddls_image_end_kernel, recovery form       g = (2 / P)(gout - x*) [+ g_x] through the tanh; no z2, no noise
//   cddls_latent_update_kernel, Adam form       m, v, z in place with the clamp; the same last-ticket step counter
//
// Noise: Philox4x32-10, key = the 64-bit seed, counter = (quad index of the element, step, stream id, 0); one counter gives
// the four normals of elements 4q .. 4q + 3 by Box-Muller (words 0, 1 -> elements 0, 1; words 2, 3 -> elements 2, 3).  A
// draw depends on (seed, stream, step, element) only, never on the launch shape.  The step is read from device memory
// (state[0]); state[1] is the arrival counter of cddls_latent_update_kernel, whose last block writes state[0] + 1 -- every
// block has read the step by then, so one captured graph serves every step and replays the eager run's bits.
//
// All kernels: one thread per quad of elements, grid-stride, 16-byte accesses when every pointer is 16-byte aligned (the
// quad that straddles the end and unaligned buffers take the scalar form), wave64, no LDS except the energy reduction.
#include "../../include/contrad_hip.h"
#include "common.h"

namespace {

// stream ids of the counter (include/contrad_hip.h; contrad_amd/cddls.py passes CD_STREAM_INIT's value to the fill entry)
enum CddlsStream { CD_STREAM_Z = 0, CD_STREAM_Z2 = 1, CD_STREAM_INIT = 2 };

constexpr int CD_THREADS = 256;
constexpr int CD_MAX_BLOCKS = 2048;      // 8 blocks per CU: enough loads in flight for an HBM stream, grid-stride beyond

__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// -log(u), u = ((w >> 8) + 0.5) * 2^-24 = (2x + 1) * 2^-25 in (0, 1), without rounding u: below one half 2x + 1 is a 24-bit
// integer; above, 1 - u = (2^25 - 2x - 1) * 2^-25 is one, and log1pf keeps the small results (radius near 0) accurate.
__device__ __forceinline__ float neg_log_uniform(unsigned w) {
  const unsigned x = w >> 8;
  if (x < (1u << 23)) return -logf((float)(2u * x + 1u) * 0x1p-25f);
  return -log1pf(-(float)((1u << 25) - 2u * x - 1u) * 0x1p-25f);
}

__device__ __forceinline__ void box_muller4(const unsigned w[4], float n[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float r = sqrtf(2.f * neg_log_uniform(w[2 * h]));
    const float u = ((float)(w[2 * h + 1] >> 8) + 0.5f) * 0x1p-24f;    // the angle tolerates the rounding (2 pi 2^-25 rad)
    float s, c;
    sincospif(2.f * u, &s, &c);
    n[2 * h] = r * c;
    n[2 * h + 1] = r * s;
  }
}

__device__ __forceinline__ void philox_words(long long quad, int step, int stream_id, long long seed, unsigned w[4]) {
  w[0] = (unsigned)quad; w[1] = (unsigned)step; w[2] = (unsigned)stream_id; w[3] = 0u;
  philox4x32_10(w, (unsigned)((unsigned long long)seed & 0xffffffffull), (unsigned)((unsigned long long)seed >> 32));
}

__device__ __forceinline__ void load4(const float* __restrict__ p, long long i, long long n, bool vec, float v[4]) {
  if (vec && i + 3 < n) {
    const float4 t = *reinterpret_cast<const float4*>(p + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (i + k < n) ? p[i + k] : 0.f;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ p, long long i, long long n, bool vec, const float v[4]) {
  if (vec && i + 3 < n) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) p[i + k] = v[k];
  }
}

// the step's normals of quad q: explicit buffer (tests) or the generator
__device__ __forceinline__ void noise4(const float* __restrict__ noise, long long q, long long n, bool vec, int step,
                                       int stream_id, long long seed, float v[4]) {
  if (noise) {
    load4(noise, 4 * q, n, vec, v);
  } else {
    unsigned w[4];
    philox_words(q, step, stream_id, seed, w);
    box_muller4(w, v);
  }
}

__global__ __launch_bounds__(CD_THREADS) void cddls_normal_fill_kernel(float* __restrict__ out,
                                                                       unsigned* __restrict__ words, long long n,
                                                                       long long seed, int stream_id,
                                                                       const int* __restrict__ step_dev, int step,
                                                                       int vec) {
  const int st = step_dev ? step_dev[0] : step;
  const long long nq = (n + 3) / 4;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
    unsigned w[4];
    float v[4];
    philox_words(q, st, stream_id, seed, w);
    box_muller4(w, v);
    if (out) store4(out, 4 * q, n, vec != 0, v);
    if (words) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * q + k < n) words[4 * q + k] = w[k];
    }
  }
}

// The three index forms of the join kernel (the arithmetic is one: (first + second) * lrelu'(act)); `form` is a launch
// argument, so the branch between them is wave-uniform and each loop keeps its own registers.  Any values and any order of
// the tests are correct.  These were kept because, with the compiler this was developed on, they put the seed loop right
// behind the entry block; nothing checks that layout, and that it is worth anything to the ~10 us seed launch is only
// supposed.
enum CddlsJoinForm { CD_FORM_JOIN = 0, CD_FORM_POOLED = 1, CD_FORM_SEED = 2 };

__device__ __forceinline__ float4 lrelu_bwd4(const float4 s, const float4 a, float slope) {
  float4 o;
  o.x = s.x * (a.x > 0.f ? 1.f : slope);
  o.y = s.y * (a.y > 0.f ? 1.f : slope);
  o.z = s.z * (a.z > 0.f ? 1.f : slope);
  o.w = s.w * (a.w > 0.f ? 1.f : slope);
  return o;
}

// seed: act / out (N, F); first g[n][f], second the row c[f]
__device__ __forceinline__ void join_seed_form(const float* g_head, const float* __restrict__ c_row,
                                               const float* __restrict__ act, float* out, long long N, int F,
                                               float slope, long long q0, long long stride) {
  const int fq = F / 4;
  const long long nq = N * fq;
  for (long long q = q0; q < nq; q += stride) {
    const int j = (int)(q % fq);
    const float4 g = *reinterpret_cast<const float4*>(g_head + 4 * q);
    const float4 c = *reinterpret_cast<const float4*>(c_row + 4 * j);
    const float4 a = *reinterpret_cast<const float4*>(act + 4 * q);
    *reinterpret_cast<float4*>(out + 4 * q) = lrelu_bwd4(make_float4(g.x + c.x, g.y + c.y, g.z + c.z, g.w + c.w), a, slope);
  }
}

// pooled seed: act / out (N, T, C) NHWC-flat; first g[n][c] spread over the T pixels of an average pool, second the row c[c]
__device__ __forceinline__ void join_pooled_form(const float* __restrict__ g, const float* __restrict__ c_row,
                                                 const float* __restrict__ act, float* __restrict__ out, long long N,
                                                 int T, int C, float slope, long long q0, long long stride) {
  const int cq = C / 4;
  const long long per = (long long)T * cq, nq = N * per;
  const float inv_T = 1.0f / (float)T;
  for (long long q = q0; q < nq; q += stride) {
    const long long n = q / per;
    const int j = (int)((q - n * per) % cq);
    const float4 h = *reinterpret_cast<const float4*>(g + 4 * (n * cq + j));
    const float4 c = *reinterpret_cast<const float4*>(c_row + 4 * j);
    const float4 a = *reinterpret_cast<const float4*>(act + 4 * q);
    const float4 s = make_float4((h.x + c.x) * inv_T, (h.y + c.y) * inv_T, (h.z + c.z) * inv_T, (h.w + c.w) * inv_T);
    *reinterpret_cast<float4*>(out + 4 * q) = lrelu_bwd4(s, a, slope);
  }
}

// join: flat tensors of 4 nq floats; first a[i], second b[i]
__device__ __forceinline__ void join_flat_form(const float* a, const float* __restrict__ b,
                                               const float* __restrict__ act, float* out, long long nq, float slope,
                                               long long q0, long long stride) {
  for (long long q = q0; q < nq; q += stride) {
    const float4 u = *reinterpret_cast<const float4*>(a + 4 * q);
    const float4 v = *reinterpret_cast<const float4*>(b + 4 * q);
    const float4 x = *reinterpret_cast<const float4*>(act + 4 * q);
    *reinterpret_cast<float4*>(out + 4 * q) = lrelu_bwd4(make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w), x, slope);
  }
}

// out may be `first` in the seed and join forms (every quad is read before it is written, by the thread that writes it)
__global__ __launch_bounds__(CD_THREADS) void cddls_feature_seed_kernel(const float* first,
                                                                        const float* __restrict__ second,
                                                                        const float* __restrict__ act, float* out,
                                                                        long long N, int T, int F, float slope,
                                                                        int form) {
  // F % 4 == 0 and 16-byte aligned bases (checked by the launchers): a quad never straddles two rows or two pixels
  // the launch geometry is read once, ahead of the branch: read inside each form, the block size became a dependent vector
  // load at the head of every form (0.6 us on the 10.7 us seed launch)
  const long long q0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
  if (form == CD_FORM_POOLED) {
    join_pooled_form(first, second, act, out, N, T, F, slope, q0, stride);
  } else if (form == CD_FORM_SEED) {
    join_seed_form(first, second, act, out, N, F, slope, q0, stride);
  } else {
    join_flat_form(first, second, act, out, N, slope, q0, stride);        // N: the quad count
  }
}

// y / dy: rows of stride ldy in the layout bn_relu_apply WROTE (perm_hw > 1: column c = ch * perm_hw + hw of x sits at
// hw * (K / perm_hw) + ch); dx: rows of stride ldx in x's own column order.
__global__ __launch_bounds__(CD_THREADS) void cddls_bn_relu_bwd_eval_kernel(const float* dy,
                                                                            const float* __restrict__ y, float* dx,
                                                                            long long M, int K, int ldy, int ldx,
                                                                            const float* __restrict__ gamma,
                                                                            const float* __restrict__ var, float eps,
                                                                            int perm_hw, int vec) {
  if (vec) {                        // perm_hw == 1, K % 4 == 0, both strides % 4 == 0, aligned bases
    const int kq = K / 4;
    const long long nq = M * kq;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
      const long long r = q / kq;
      const int c = (int)(q - r * kq) * 4;
      const float4 g = *reinterpret_cast<const float4*>(dy + r * ldy + c);
      const float4 a = *reinterpret_cast<const float4*>(y + r * ldy + c);
      const float4 gm = *reinterpret_cast<const float4*>(gamma + c);
      const float4 vr = *reinterpret_cast<const float4*>(var + c);
      float4 o;
      o.x = a.x > 0.f ? g.x * (gm.x * rsqrtf(vr.x + eps)) : 0.f;
      o.y = a.y > 0.f ? g.y * (gm.y * rsqrtf(vr.y + eps)) : 0.f;
      o.z = a.z > 0.f ? g.z * (gm.z * rsqrtf(vr.z + eps)) : 0.f;
      o.w = a.w > 0.f ? g.w * (gm.w * rsqrtf(vr.w + eps)) : 0.f;
      *reinterpret_cast<float4*>(dx + r * ldx + c) = o;
    }
    return;
  }
  const long long total = M * K;
  const int nch = K / perm_hw;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / K;
    const int p = (int)(e - r * K);                     // position in y's layout: consecutive lanes read consecutive floats
    int c = p;
    if (perm_hw > 1) {
      const int hw = p / nch, ch = p - hw * nch;
      c = ch * perm_hw + hw;
    }
    const float g = dy[r * ldy + p];
    dx[r * ldx + c] = y[r * ldy + p] > 0.f ? g * (gamma[c] * rsqrtf(var[c] + eps)) : 0.f;
  }
}

__global__ __launch_bounds__(CD_THREADS) void cddls_compose_kernel(const float* __restrict__ gout,
                                                                   const float* __restrict__ z2, float* __restrict__ x,
                                                                   long long n, float eps, int clamp01, int vec) {
  const long long nq = (n + 3) / 4;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
    float g[4], b[4], o[4];
    load4(gout, 4 * q, n, vec != 0, g);
    load4(z2, 4 * q, n, vec != 0, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = fmaf(eps, b[k], g[k]);
      if (clamp01) o[k] = fminf(fmaxf(o[k], 0.f), 1.f);
    }
    store4(x, 4 * q, n, vec != 0, o);
  }
}

// recovery form of the image end: the loss's own pixel gradient (scale = 2 / P) plus the D half's (gx, may be null),
// through the tanh.  No z2, no noise, no Philox work.
__device__ __forceinline__ void image_end_recover_form(const float* __restrict__ gx, const float* __restrict__ gout,
                                                       const float* __restrict__ target, float* __restrict__ g_lin,
                                                       long long n, float scale, bool vec, long long q0,
                                                       long long stride) {
  const long long nq = (n + 3) / 4;
  for (long long q = q0; q < nq; q += stride) {
    float g[4] = {0.f, 0.f, 0.f, 0.f}, o[4], x[4], gl[4];
    if (gx) load4(gx, 4 * q, n, vec, g);
    load4(gout, 4 * q, n, vec, o);
    load4(target, 4 * q, n, vec, x);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float t = 2.f * o[k] - 1.f;
      gl[k] = fmaf(scale, o[k] - x[k], g[k]) * (0.5f * (1.f - t * t));
    }
    store4(g_lin, 4 * q, n, vec, gl);
  }
}

__global__ __launch_bounds__(CD_THREADS) void cddls_image_end_kernel(const float* __restrict__ gx,
                                                                     const float* __restrict__ gout, float* z2,
                                                                     float* __restrict__ g_lin, long long n, float eps,
                                                                     float noise_scale, const float* __restrict__ noise,
                                                                     long long seed, const int* __restrict__ state,
                                                                     int vec, const float* __restrict__ target,
                                                                     float target_scale) {
  // the launch geometry is read once, ahead of the branch; the Langevin loop stays right behind the entry block and the
  // recovery form (target != null: a launch argument, wave-uniform) behind it
  const long long q0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
  if (__builtin_expect(target == nullptr, 1)) {
    const int step = state ? state[0] : 0;
    const float he = 0.5f * eps;
    const long long nq = (n + 3) / 4;
    for (long long q = q0; q < nq; q += stride) {
      float g[4], o[4], b[4], nz[4], gl[4];
      load4(gx, 4 * q, n, vec != 0, g);
      load4(gout, 4 * q, n, vec != 0, o);
      load4(z2, 4 * q, n, vec != 0, b);
      noise4(noise, q, n, vec != 0, step, CD_STREAM_Z2, seed, nz);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float t = 2.f * o[k] - 1.f;                     // tanh of the generator's last pre-activation
        gl[k] = g[k] * (0.5f * (1.f - t * t));
        const float gz2 = fmaf(eps, g[k], b[k]);              // d e / d z2 = eps * g_x + z2
        b[k] = fmaf(noise_scale, nz[k], fmaf(-he, gz2, b[k]));
      }
      store4(g_lin, 4 * q, n, vec != 0, gl);
      store4(z2, 4 * q, n, vec != 0, b);
    }
  } else {
    image_end_recover_form(gx, gout, target, g_lin, n, target_scale, vec != 0, q0, stride);
  }
}

// Adam form of the latent update, t = step + 1:  m <- b1 m + (1 - b1) g,  v <- b2 v + (1 - b2) g^2,
// z <- clamp(z - lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + adam_eps), -1, 1).  The two bias corrections are made once
// per thread in float64 and rounded once to fp32.  g = 0 on m = v = 0 leaves z bitwise as it was.
__device__ __forceinline__ void latent_adam_form(float* z, const float* __restrict__ gz, float* m, float* v, long long n,
                                                 float lr, float b1, float b2, float adam_eps, int step, bool vec,
                                                 long long q0, long long stride) {
  const double t = (double)step + 1.0;
  const float c1 = (float)(1.0 - pow((double)b1, t)), c2 = (float)(1.0 - pow((double)b2, t));
  const float ob1 = 1.f - b1, ob2 = 1.f - b2;
  const long long nq = (n + 3) / 4;
  for (long long q = q0; q < nq; q += stride) {
    float a[4], g[4], mm[4], vv[4];
    load4(z, 4 * q, n, vec, a);
    load4(gz, 4 * q, n, vec, g);
    load4(m, 4 * q, n, vec, mm);
    load4(v, 4 * q, n, vec, vv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mm[k] = fmaf(b1, mm[k], ob1 * g[k]);
      vv[k] = fmaf(b2, vv[k], ob2 * (g[k] * g[k]));
      const float u = (mm[k] / c1) / (sqrtf(vv[k] / c2) + adam_eps);
      a[k] = fminf(fmaxf(fmaf(-lr, u, a[k]), -1.f), 1.f);
    }
    store4(m, 4 * q, n, vec, mm);
    store4(v, 4 * q, n, vec, vv);
    store4(z, 4 * q, n, vec, a);
  }
}

__global__ __launch_bounds__(CD_THREADS) void cddls_latent_update_kernel(float* z, const float* __restrict__ gz,
                                                                         long long n, float eps, float noise_scale,
                                                                         const float* __restrict__ noise,
                                                                         long long seed, int* state, int vec, float* m,
                                                                         float* v, float b1, float b2, float adam_eps) {
  const int step = state ? state[0] : 0;
  if (__builtin_expect(m != nullptr, 0)) {        // wave-uniform: a launch argument (eps carries the learning rate)
    latent_adam_form(z, gz, m, v, n, eps, b1, b2, adam_eps, step, vec != 0,
                     (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
  } else {
    const float he = 0.5f * eps;
    const long long nq = (n + 3) / 4;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
      float a[4], g[4], nz[4];
      load4(z, 4 * q, n, vec != 0, a);
      load4(gz, 4 * q, n, vec != 0, g);
      noise4(noise, q, n, vec != 0, step, CD_STREAM_Z, seed, nz);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float u = fmaf(noise_scale, nz[k], fmaf(-he, g[k], a[k]));
        a[k] = fminf(fmaxf(u, -1.f), 1.f);
      }
      store4(z, 4 * q, n, vec != 0, a);
    }
  }
  if (state == nullptr) return;
  // every thread of this block has read state[0] (the value is in a register before the barrier); the block that draws
  // the last ticket knows that all the others have too
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = __hip_atomic_fetch_add(state + 1, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t == (int)gridDim.x - 1) {
      __hip_atomic_store(state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(state, step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// recovery form of the energy kernel: pix[n] = |gout[n] - x*[n]|^2 / P, feat[n] = |phi[n] - phi*[n]|^2 / F (0 without phi), loss[n] = pix[n] +
// lam feat[n], and the residual row r[n][f] = (2 lam / F)(phi - phi*).  One block per sample, the sums in the order of the
// Langevin form (a strided partial per lane, the wave tree, the waves in index order): no atomics, two calls bitwise equal.
__device__ __forceinline__ void energy_recover_form(const float* __restrict__ gout, const float* __restrict__ target,
                                                    const float* __restrict__ phi, const float* __restrict__ phi_target,
                                                    float* __restrict__ resid, float* __restrict__ pix,
                                                    float* __restrict__ featl, float* __restrict__ loss, int F,
                                                    long long P, float lam, float* red) {
  const long long n = blockIdx.x;
  const float* o = gout + n * P;
  const float* x = target + n * P;
  float q = 0.f, s = 0.f;
  for (long long i = threadIdx.x; i < P; i += blockDim.x) {
    const float d = o[i] - x[i];
    q = fmaf(d, d, q);
  }
  q = block_sum(q, red);
  if (phi) {                        // block-uniform
    const float* f = phi + n * F;
    const float* t = phi_target + n * F;
    float* r = resid + n * F;
    const float rs = (2.f * lam) / (float)F;
    for (int i = threadIdx.x; i < F; i += blockDim.x) {
      const float d = f[i] - t[i];
      s = fmaf(d, d, s);
      r[i] = rs * d;
    }
    s = block_sum(s, red);
  }
  if (threadIdx.x == 0) {
    const float pv = q / (float)P, fv = phi ? s / (float)F : 0.f;
    pix[n] = pv;
    featl[n] = fv;
    loss[n] = fmaf(lam, fv, pv);
  }
}

// e[n] = -d[n] + <feat[n], c_row> + bias_term[0] + 0.5 |z2[n]|^2 with c_row = -lbd * w_y (trunk order), bias_term = -lbd * b_y
__global__ __launch_bounds__(CD_THREADS) void cddls_energy_kernel(const float* __restrict__ d, int ldd,
                                                                  const float* __restrict__ feat,
                                                                  const float* __restrict__ c_row,
                                                                  const float* __restrict__ bias_term,
                                                                  const float* __restrict__ z2, float* __restrict__ e,
                                                                  int F, long long P,
                                                                  const float* __restrict__ target,
                                                                  float* __restrict__ resid, float* __restrict__ pix,
                                                                  float* __restrict__ featl, float lam) {
  __shared__ float red[16];
  if (__builtin_expect(target == nullptr, 1)) {       // the Langevin form stays right behind the entry block
    const long long n = blockIdx.x;
    const float* f = feat + n * F;
    const float* b = z2 + n * P;
    float s = 0.f, q = 0.f;
    for (int i = threadIdx.x; i < F; i += blockDim.x) s = fmaf(f[i], c_row[i], s);
    for (long long i = threadIdx.x; i < P; i += blockDim.x) q = fmaf(b[i], b[i], q);
    s = block_sum(s, red);
    q = block_sum(q, red);
    if (threadIdx.x == 0) e[n] = (s + bias_term[0] - d[n * ldd]) + 0.5f * q;
  } else {            // wave-uniform: a launch argument (z2 = gout, feat = phi, c_row = phi*, e = loss)
    energy_recover_form(z2, target, feat, c_row, resid, pix, featl, e, F, P, lam, red);
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int quad_grid(long long quads) {
  long long g = (quads + CD_THREADS - 1) / CD_THREADS;
  if (g < 1) g = 1;
  return (int)(g > CD_MAX_BLOCKS ? CD_MAX_BLOCKS : g);
}

inline float noise_scale_of(float eps, float sigma_n) { return (float)((double)sigma_n * sqrt((double)eps)); }

}  // namespace

extern "C" int contrad_cddls_normal_fill(float* out, unsigned* words, long long n, long long seed, int stream_id,
                                         const void* step_dev, int step, int grid_blocks, contrad_stream_t stream) {
  CONTRAD_ARG((out || words) && n >= 1 && stream_id >= 0 && grid_blocks >= 0 && grid_blocks <= 65536);
  const int grid = grid_blocks > 0 ? grid_blocks : quad_grid((n + 3) / 4);
  hipLaunchKernelGGL(cddls_normal_fill_kernel, dim3(grid), dim3(CD_THREADS), 0, (hipStream_t)stream, out, words, n, seed,
                     stream_id, static_cast<const int*>(step_dev), step, (int)(out == nullptr || al16(out)));
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_feature_seed(const float* g_head, const float* c_row, const float* act, float* out,
                                          long long N, int F, float slope, contrad_stream_t stream) {
  CONTRAD_ARG(g_head && c_row && act && out && N >= 1 && F >= 4 && (F & 3) == 0);
  CONTRAD_ARG(al16(g_head) && al16(c_row) && al16(act) && al16(out));
  hipLaunchKernelGGL(cddls_feature_seed_kernel, dim3(quad_grid(N * (F / 4))), dim3(CD_THREADS), 0, (hipStream_t)stream,
                     g_head, c_row, act, out, N, 1, F, slope, (int)CD_FORM_SEED);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_pooled_seed(const float* g, const float* c_row, const float* act, float* out, long long N,
                                         int T, int C, float slope, contrad_stream_t stream) {
  CONTRAD_ARG(g && c_row && act && out && out != g && N >= 1 && T >= 1 && C >= 4 && (C & 3) == 0);
  CONTRAD_ARG(al16(g) && al16(c_row) && al16(act) && al16(out));
  hipLaunchKernelGGL(cddls_feature_seed_kernel, dim3(quad_grid(N * T * (C / 4))), dim3(CD_THREADS), 0,
                     (hipStream_t)stream, g, c_row, act, out, N, T, C, slope, (int)CD_FORM_POOLED);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_join_bwd(const float* a, const float* b, const float* act, float* out, long long n,
                                      float slope, contrad_stream_t stream) {
  CONTRAD_ARG(a && b && act && out && n >= 1 && (n & 3) == 0);
  CONTRAD_ARG(al16(a) && al16(b) && al16(act) && al16(out));
  hipLaunchKernelGGL(cddls_feature_seed_kernel, dim3(quad_grid(n / 4)), dim3(CD_THREADS), 0, (hipStream_t)stream, a, b,
                     act, out, n / 4, 1, 4, slope, (int)CD_FORM_JOIN);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_bn_relu_bwd_eval(const float* dy, const float* y, float* dx, long long M, int K, int ldy,
                                              int ldx, const float* gamma, const float* running_var, float eps,
                                              int perm_hw, contrad_stream_t stream) {
  CONTRAD_ARG(dy && y && dx && gamma && running_var && M >= 1 && K >= 1 && ldy >= K && ldx >= K);
  CONTRAD_ARG(perm_hw >= 1 && K % perm_hw == 0);
  CONTRAD_ARG(perm_hw == 1 || (dx != dy && dx != y));          // the permuted form is not an in-place map
  const int vec = perm_hw == 1 && (K & 3) == 0 && (ldy & 3) == 0 && (ldx & 3) == 0 && al16(dy) && al16(y) && al16(dx) &&
                  al16(gamma) && al16(running_var);
  const long long items = vec ? M * (K / 4) : M * K;
  hipLaunchKernelGGL(cddls_bn_relu_bwd_eval_kernel, dim3(quad_grid(items)), dim3(CD_THREADS), 0, (hipStream_t)stream, dy,
                     y, dx, M, K, ldy, ldx, gamma, running_var, eps, perm_hw, vec);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_compose(const float* gout, const float* z2, float* x, long long n, float eps, int clamp01,
                                     contrad_stream_t stream) {
  CONTRAD_ARG(gout && z2 && x && n >= 1);
  hipLaunchKernelGGL(cddls_compose_kernel, dim3(quad_grid((n + 3) / 4)), dim3(CD_THREADS), 0, (hipStream_t)stream, gout,
                     z2, x, n, eps, clamp01, (int)(al16(gout) && al16(z2) && al16(x)));
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_image_end(const float* gx, const float* gout, float* z2, float* g_lin, long long n,
                                       float eps, float sigma_n, const float* noise, long long seed, const void* state,
                                       contrad_stream_t stream) {
  CONTRAD_ARG(gx && gout && z2 && g_lin && n >= 1 && eps >= 0.f);
  const int vec = al16(gx) && al16(gout) && al16(z2) && al16(g_lin) && (noise == nullptr || al16(noise));
  hipLaunchKernelGGL(cddls_image_end_kernel, dim3(quad_grid((n + 3) / 4)), dim3(CD_THREADS), 0, (hipStream_t)stream, gx,
                     gout, z2, g_lin, n, eps, noise_scale_of(eps, sigma_n), noise, seed, static_cast<const int*>(state), vec,
                     (const float*)nullptr, 0.f);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_latent_update(float* z, const float* gz, long long n, float eps, float sigma_n,
                                           const float* noise, long long seed, void* state, contrad_stream_t stream) {
  CONTRAD_ARG(z && gz && n >= 1 && eps >= 0.f);
  const int vec = al16(z) && al16(gz) && (noise == nullptr || al16(noise));
  hipLaunchKernelGGL(cddls_latent_update_kernel, dim3(quad_grid((n + 3) / 4)), dim3(CD_THREADS), 0, (hipStream_t)stream,
                     z, gz, n, eps, noise_scale_of(eps, sigma_n), noise, seed, static_cast<int*>(state), vec, (float*)nullptr,
                     (float*)nullptr, 0.f, 0.f, 0.f);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_energy(const float* d, int ldd, const float* feat, const float* c_row,
                                    const float* bias_term, const float* z2, float* e, int N, int F, long long P,
                                    contrad_stream_t stream) {
  CONTRAD_ARG(d && feat && c_row && bias_term && z2 && e && N >= 1 && F >= 1 && P >= 1 && ldd >= 1);
  hipLaunchKernelGGL(cddls_energy_kernel, dim3(N), dim3(CD_THREADS), 0, (hipStream_t)stream, d, ldd, feat, c_row,
                     bias_term, z2, e, F, P, (const float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.f);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

// ---- latent recovery (contrad_amd/recover.py): the recovery / Adam forms of the three kernels above ----
extern "C" int contrad_cddls_recover_loss(const float* gout, const float* target, const float* phi,
                                          const float* phi_target, float* resid, float* pix, float* feat, float* loss,
                                          int N, int F, long long P, float lambda_feat, contrad_stream_t stream) {
  CONTRAD_ARG(gout && target && pix && feat && loss && N >= 1 && P >= 1);
  CONTRAD_ARG(phi ? (phi_target && resid && F >= 1) : (!phi_target && !resid));
  hipLaunchKernelGGL(cddls_energy_kernel, dim3(N), dim3(CD_THREADS), 0, (hipStream_t)stream, (const float*)nullptr, 1, phi,
                     phi_target, (const float*)nullptr, gout, loss, F, P, target, resid, pix, feat, lambda_feat);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_recover_image_end(const float* gx, const float* gout, const float* target, float* g_lin,
                                               long long n, long long P, contrad_stream_t stream) {
  CONTRAD_ARG(gout && target && g_lin && n >= 1 && P >= 1);
  const int vec = (gx == nullptr || al16(gx)) && al16(gout) && al16(target) && al16(g_lin);
  hipLaunchKernelGGL(cddls_image_end_kernel, dim3(quad_grid((n + 3) / 4)), dim3(CD_THREADS), 0, (hipStream_t)stream, gx,
                     gout, (float*)nullptr, g_lin, n, 0.f, 0.f, (const float*)nullptr, 0ll, (const int*)nullptr, vec, target,
                     (float)(2.0 / (double)P));
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_cddls_recover_update(float* z, const float* gz, float* m, float* v, long long n, float lr,
                                            float beta1, float beta2, float adam_eps, void* state,
                                            contrad_stream_t stream) {
  CONTRAD_ARG(z && gz && m && v && state && n >= 1 && lr >= 0.f);
  CONTRAD_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && adam_eps >= 0.f);
  const int vec = al16(z) && al16(gz) && al16(m) && al16(v);
  hipLaunchKernelGGL(cddls_latent_update_kernel, dim3(quad_grid((n + 3) / 4)), dim3(CD_THREADS), 0, (hipStream_t)stream,
                     z, gz, n, lr, 0.f, (const float*)nullptr, 0ll, static_cast<int*>(state), vec, m, v, beta1, beta2,
                     adam_eps);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
