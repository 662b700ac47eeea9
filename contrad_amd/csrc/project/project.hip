// StyleGAN2 projector (gfx950): the device side of contrad_amd/project.py -- the loss ends of projecting an image
// onto the generator that are not convolutions.
//
//   image_end        x, t fp32 [N][3][H][W] -> the rows pix_l[n] = mean(pool_l(x - t)^2), l < L <= 4 (pool_l the 2^l x 2^l mean), and
//                    g_x = d sum_n sum_l lam_l pix_l[n] / d x = (2 / 3HW) sum_l lam_l pool_l(x - t)[tile of the pixel] (pool_l is
//                    linear, and its adjoint's 4^-l cancels against the 4^l in 1 / (3 H W / 4^l)).  One workgroup owns a band of
//                    rows of one channel plane (a multiple of T = 2^(L-1) rows, about 4096 values): the residual is formed once
//                    in LDS, every pooled level from the level below it (((a + b) + (c + d)) / 4), the gradient from the LDS
//                    levels.  Squares are added per thread in index order (stride 256), then wave butterfly, then the four wave
//                    sums in order, into partial[l][n][band]; a second launch adds the bands of an image, one wave per (l, n).
//   noise_grad       g fp32 [P][K] (NHWC rows) -> out[p] = noise_w sum_k g[p][k].  LP = the power of two >= K / 4 (at most 64)
//                    lanes share a pixel and read its row as float4 in strides of LP: 8 channels are two lanes, so a wave reads 32
//                    pixels = 1 KiB contiguous; 512 channels are two float4 per lane.  The lanes of a pixel are added by a butterfly
//                    of log2 LP steps.  Rows that are no multiple of four floats (or a base off 16 bytes) take the scalar form.
//   noise_reg        one map set [N][1][R][R], R a power of two in [4, 1024] -> reg[n] = sum_j a_j^2 + b_j^2 over the levels
//                    m_0 = map, m_{j+1} = avgpool2(m_j) down to the first of side <= 8, a_j = mean(m_j roll(m_j, 1, W)),
//                    b_j = mean(m_j roll(m_j, 1, H)) (circular), and gacc += scale * d reg[n] / d map, which is
//                    (2 / R^2) sum_j a_j (m_j[y][x-1] + m_j[y][x+1]) + b_j (m_j[y-1][x] + m_j[y+1][x]) at (y, x) = (h, w) >> j.
//                    Four launches on caller-owned scratch: the pyramid (one workgroup pools a 128 x 128 tile down to 1 x 1 through
//                    LDS, reading 2 x 2 quads of the map as float2 pairs), the products (4096 values of one level per workgroup
//                    -> two partial sums), the finish (one wave per image: a_j, b_j, reg) and the gradient (one thread per pixel).
//   noise_normalize  in place per image: m -= mean(m), m *= 1 / sqrt(mean(m^2)); a map whose centred square mean is 0 becomes
//                    zeros.  The mean is formed about the map's first element (mean = m[0] + mean(m - m[0])), so a constant map
//                    is centred to exact zeros whatever its value.  One workgroup per image, three passes (the map stays in L2).
// fp32 storage and accumulation; every sum has a fixed order and no atomics: two calls are bitwise equal.
#include "../../../include/contrad_hip.h"
#include "../common.h"

#include <stdint.h>

namespace {

constexpr int PROJ_THREADS = 256;
constexpr int IMG_BAND_VALUES = 4096;       // values of one channel plane per workgroup of image_end (LDS: at most 4/3 of it)
constexpr int IMG_MAX_BAND = 8192;          // T * W may reach this when one T-row band is already longer than IMG_BAND_VALUES
constexpr int REG_TILE = 128;               // side of the map tile one workgroup pools
constexpr int REG_CHUNK = 4096;             // values of one level per workgroup of the product sums
constexpr int REG_MAX_LEVELS = 8;           // R = 1024: 1024, 512, ..., 8
constexpr int REG_LDS_FLOATS = 5464;        // 64^2 + 32^2 + ... + 1 = 5461

struct Lam4 {
  float v[4];
};

__device__ __forceinline__ float pool4(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

// ---- image_end ----
__global__ void __launch_bounds__(PROJ_THREADS) image_end_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                 float* __restrict__ gx, float* __restrict__ partial, Lam4 lam, int L,
                                                                 int N, int H, int W, int rows, float gscale) {
  extern __shared__ __attribute__((aligned(16))) float lds[];       // level l at lvl[l]: (rows >> l) x (W >> l)
  __shared__ float red[16];
  const int band = blockIdx.x, c = blockIdx.y, n = blockIdx.z, bands = gridDim.x;
  const int tid = threadIdx.x;
  const long long base = (((long long)n * 3 + c) * H + (long long)band * rows) * W;
  float* lvl[4];
  lvl[0] = lds;
  for (int l = 1; l < 4; ++l) lvl[l] = lvl[l - 1] + (rows >> (l - 1)) * (W >> (l - 1));
  const int count = rows * W;
  for (int i = tid; i < count; i += PROJ_THREADS) lds[i] = x[base + i] - t[base + i];
  __syncthreads();
  for (int l = 1; l < L; ++l) {
    const int Wl = W >> l, Wp = W >> (l - 1), cnt = (rows >> l) * Wl;
    const float* src = lvl[l - 1];
    float* dst = lvl[l];
    for (int i = tid; i < cnt; i += PROJ_THREADS) {
      const int y = i / Wl, xq = i - y * Wl;
      const float* p = src + (2 * y) * Wp + 2 * xq;
      dst[i] = pool4(p[0], p[1], p[Wp], p[Wp + 1]);
    }
    __syncthreads();
  }
  const int nb = 3 * bands;
  for (int l = 0; l < L; ++l) {
    const int cnt = (rows >> l) * (W >> l);
    const float* src = lvl[l];
    float s = 0.f;
    for (int i = tid; i < cnt; i += PROJ_THREADS) s += src[i] * src[i];
    s = block_sum(s, red);
    if (tid == 0) partial[((long long)l * N + n) * nb + c * bands + band] = s;
  }
  for (int i = tid; i < count; i += PROJ_THREADS) {
    const int row = i / W, col = i - row * W;
    float acc = 0.f;
    for (int l = 0; l < L; ++l) acc += lam.v[l] * lvl[l][(row >> l) * (W >> l) + (col >> l)];
    gx[base + i] = gscale * acc;
  }
}

// pix[l][n] = (the bands of image n at level l, in order) / P_l; one wave per (l, n)
__global__ void __launch_bounds__(64) image_end_finish_kernel(const float* __restrict__ partial, float* __restrict__ pix, int N, int nb,
                                                              float p0) {
  const int ln = blockIdx.x, l = ln / N;
  const float* p = partial + (long long)ln * nb;
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 64) s += p[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) pix[ln] = s / (p0 / (float)(1 << (2 * l)));
}

// ---- noise_grad ----
template <bool VEC>
__global__ void __launch_bounds__(PROJ_THREADS) noise_grad_kernel(const float* __restrict__ g, const float* __restrict__ noise_w,
                                                                  float* __restrict__ out, long long P, int K, int lpshift) {
  const long long gid = (long long)blockIdx.x * PROJ_THREADS + threadIdx.x;
  const long long pix = gid >> lpshift;
  const int LP = 1 << lpshift, sub = (int)(gid & (LP - 1));
  float s = 0.f;
  if (pix < P) {
    const float* row = g + pix * K;
    if (VEC) {
      const float4* row4 = reinterpret_cast<const float4*>(row);
      for (int q = sub; q < (K >> 2); q += LP) {
        const float4 v = row4[q];
        s += (v.x + v.y) + (v.z + v.w);
      }
    } else {
      for (int k = sub; k < K; k += LP) s += row[k];
    }
  }
  for (int o = LP >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);   // (every lane of the wave takes part: no early return above)
  if (pix < P && sub == 0) out[pix] = noise_w[0] * s;
}

// ---- noise_reg ----
struct RegPlan {
  int J;                 // levels
  int nblk0;             // workgroups of the product sums at level 0 (the stride of the partial sums of every level)
  long long pyr;         // floats of the levels 1 .. J - 1 of one image
  long long off[REG_MAX_LEVELS];      // offset of level j >= 1 inside an image's pyramid
};

RegPlan reg_plan(int R) {
  RegPlan p;
  p.J = 1;
  for (int s = R; s > 8; s >>= 1) ++p.J;
  p.nblk0 = (int)cdivll((long long)R * R, REG_CHUNK);
  p.pyr = 0;
  p.off[0] = 0;
  for (int j = 1; j < p.J; ++j) {
    p.off[j] = p.pyr;
    p.pyr += (long long)(R >> j) * (R >> j);
  }
  for (int j = p.J; j < REG_MAX_LEVELS; ++j) p.off[j] = 0;
  return p;
}

struct RegOff {
  long long v[REG_MAX_LEVELS];
};

// the levels 1 .. J - 1 of one T x T tile (T = min(R, 128)), written to pyr[n]
__global__ void __launch_bounds__(PROJ_THREADS) reg_pyramid_kernel(const float* __restrict__ map, float* __restrict__ pyr, RegOff off,
                                                                   long long pyr_n, int R, int T, int J) {
  __shared__ __attribute__((aligned(16))) float lds[REG_LDS_FLOATS];
  const int tiles = R / T, ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles, n = blockIdx.y;
  const int tid = threadIdx.x;
  const float* m = map + (long long)n * R * R;
  float* out = pyr + (long long)n * pyr_n;
  {
    const int S = T >> 1, Rl = R >> 1;
    for (int q = tid; q < S * S; q += PROJ_THREADS) {
      const int qy = q / S, qx = q - qy * S;
      const float* p = m + (long long)(ty * T + 2 * qy) * R + tx * T + 2 * qx;
      const float2 r0 = *reinterpret_cast<const float2*>(p), r1 = *reinterpret_cast<const float2*>(p + R);
      const float v = pool4(r0.x, r0.y, r1.x, r1.y);
      lds[q] = v;
      out[off.v[1] + (long long)(ty * S + qy) * Rl + tx * S + qx] = v;
    }
  }
  __syncthreads();
  const float* src = lds;
  for (int j = 2; j < J; ++j) {
    const int S = T >> j, Sp = T >> (j - 1), Rl = R >> j;
    float* dst = const_cast<float*>(src) + Sp * Sp;
    for (int q = tid; q < S * S; q += PROJ_THREADS) {
      const int qy = q / S, qx = q - qy * S;
      const float* p = src + (2 * qy) * Sp + 2 * qx;
      const float v = pool4(p[0], p[1], p[Sp], p[Sp + 1]);
      dst[q] = v;
      out[off.v[j] + (long long)(ty * S + qy) * Rl + tx * S + qx] = v;
    }
    __syncthreads();
    src = dst;
  }
}

__device__ __forceinline__ const float* reg_level(const float* map, const float* pyr, const RegOff& off, long long pyr_n, int R, int n,
                                                  int j) {
  return j == 0 ? map + (long long)n * R * R : pyr + (long long)n * pyr_n + off.v[j];
}

// part[n][j][blk] = the sums of m m(x - 1) and m m(y - 1) over the values [blk, blk + 1) * REG_CHUNK of level j
__global__ void __launch_bounds__(PROJ_THREADS) reg_products_kernel(const float* __restrict__ map, const float* __restrict__ pyr,
                                                                    float* __restrict__ part, RegOff off, long long pyr_n, int R, int J,
                                                                    int nblk0) {
  __shared__ float red[16];
  const int blk = blockIdx.x, j = blockIdx.y, n = blockIdx.z;
  const int S = R >> j, msk = S - 1, sh = 31 - __builtin_clz(S);
  const int count = S * S;
  if (blk * REG_CHUNK >= count) return;                               // (the whole workgroup: this level has fewer chunks)
  const float* src = reg_level(map, pyr, off, pyr_n, R, n, j);
  const int end = min(count, (blk + 1) * REG_CHUNK);
  float sw = 0.f, shh = 0.f;
  for (int i = blk * REG_CHUNK + threadIdx.x; i < end; i += PROJ_THREADS) {
    const int y = i >> sh, xq = i & msk;
    const float v = src[i];
    sw += v * src[(y << sh) + ((xq - 1) & msk)];
    shh += v * src[(((y - 1) & msk) << sh) + xq];
  }
  sw = block_sum(sw, red);
  shh = block_sum(shh, red);
  if (threadIdx.x == 0) {
    float* p = part + (((long long)n * J + j) * nblk0 + blk) * 2;
    p[0] = sw;
    p[1] = shh;
  }
}

// coef[n][j] = (a_j, b_j), reg[n] = sum_j a_j^2 + b_j^2; one wave per image
__global__ void __launch_bounds__(64) reg_finish_kernel(const float* __restrict__ part, float* __restrict__ coef, float* __restrict__ reg,
                                                        int R, int J, int nblk0) {
  const int n = blockIdx.x;
  float total = 0.f;
  for (int j = 0; j < J; ++j) {
    const int S = R >> j, nb = (S * S + REG_CHUNK - 1) / REG_CHUNK;
    const float* p = part + ((long long)n * J + j) * nblk0 * 2;
    float sw = 0.f, shh = 0.f;
    for (int i = threadIdx.x; i < nb; i += 64) {
      sw += p[2 * i];
      shh += p[2 * i + 1];
    }
    const float inv = 1.0f / (float)(S * S);                          // (a power of two: exact)
    const float a = wave_sum(sw) * inv, b = wave_sum(shh) * inv;
    if (threadIdx.x == 0) {
      coef[((long long)n * J + j) * 2] = a;
      coef[((long long)n * J + j) * 2 + 1] = b;
    }
    total += a * a + b * b;
  }
  if (threadIdx.x == 0) reg[n] = total;
}

__global__ void __launch_bounds__(PROJ_THREADS) reg_grad_kernel(const float* __restrict__ map, const float* __restrict__ pyr,
                                                                const float* __restrict__ coef, float* __restrict__ gacc, RegOff off,
                                                                long long pyr_n, int R, int J, float scale) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * PROJ_THREADS + threadIdx.x;
  if (i >= R * R) return;
  const int sh0 = 31 - __builtin_clz(R);
  const int h = i >> sh0, w = i & (R - 1);
  float acc = 0.f;
  for (int j = 0; j < J; ++j) {
    const int S = R >> j, msk = S - 1, sh = sh0 - j;
    const float* src = reg_level(map, pyr, off, pyr_n, R, n, j);
    const int y = h >> j, xq = w >> j;
    const float a = coef[((long long)n * J + j) * 2], b = coef[((long long)n * J + j) * 2 + 1];
    const float swv = src[(y << sh) + ((xq - 1) & msk)] + src[(y << sh) + ((xq + 1) & msk)];
    const float shv = src[(((y - 1) & msk) << sh) + xq] + src[(((y + 1) & msk) << sh) + xq];
    acc += a * swv + b * shv;
  }
  const long long o = (long long)n * R * R + i;
  gacc[o] = gacc[o] + scale * (acc * (2.0f / (float)(R * R)));
}

// ---- noise_normalize ----
__global__ void __launch_bounds__(1024) noise_normalize_kernel(float* __restrict__ map, int count) {
  __shared__ float red[16];
  float4* m = reinterpret_cast<float4*>(map + (long long)blockIdx.x * count);
  const int n4 = count >> 2;
  const float pivot = map[(long long)blockIdx.x * count];
  const float inv = 1.0f / (float)count;                              // (a power of two: exact)
  float s = 0.f;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    const float4 v = m[i];
    s += ((v.x - pivot) + (v.y - pivot)) + ((v.z - pivot) + (v.w - pivot));
  }
  s = block_sum(s, red);
  __syncthreads();                                                    // (everyone has read the pivot before it is overwritten)
  const float mean = pivot + s * inv;
  float q = 0.f;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    const float4 v = m[i];
    const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
    q += (a * a + b * b) + (c * c + d * d);
  }
  q = block_sum(q, red) * inv;
  const float r = q > 0.f ? 1.0f / sqrtf(q) : 0.f;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    float4 v = m[i];
    v.x = (v.x - mean) * r;
    v.y = (v.y - mean) * r;
    v.z = (v.z - mean) * r;
    v.w = (v.w - mean) * r;
    m[i] = v;
  }
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

extern "C" int contrad_proj_image_end(const float* x, const float* target, const float* lam, int L, float* pix, float* gx,
                                      float* partial, long long partial_floats, int N, int H, int W, contrad_stream_t stream) {
  CONTRAD_ARG(x && target && lam && pix && gx && partial);
  CONTRAD_ARG(L >= 1 && L <= 4 && N >= 1 && N <= 65535 && H >= 1 && W >= 1);
  const int T = 1 << (L - 1);
  CONTRAD_ARG(H % T == 0 && W % T == 0);
  CONTRAD_ARG((long long)T * W <= IMG_MAX_BAND);
  CONTRAD_ARG(gx != x && gx != target);
  for (int l = 0; l < L; ++l) CONTRAD_ARG(lam[l] == lam[l] && lam[l] - lam[l] == 0.f);      // finite (host floats)
  int rows = T;
  while ((long long)rows * 2 * W <= IMG_BAND_VALUES && H % (rows * 2) == 0) rows *= 2;
  const int bands = H / rows;
  CONTRAD_ARG(partial_floats >= (long long)L * N * 3 * bands);
  Lam4 lm = {{0.f, 0.f, 0.f, 0.f}};
  size_t lds = 0;
  for (int l = 0; l < L; ++l) {
    lm.v[l] = lam[l];
    lds += (size_t)(rows >> l) * (W >> l) * sizeof(float);
  }
  const float p0 = 3.0f * (float)H * (float)W;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(image_end_kernel, dim3((unsigned)bands, 3, (unsigned)N), dim3(PROJ_THREADS), lds, st, x, target, gx, partial, lm, L,
                     N, H, W, rows, 2.0f / p0);
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(image_end_finish_kernel, dim3((unsigned)(L * N)), dim3(64), 0, st, partial, pix, N, 3 * bands, p0);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_proj_noise_grad(const float* g_pre, const float* noise_w, float* g_noise, long long P, int K,
                                       contrad_stream_t stream) {
  CONTRAD_ARG(g_pre && noise_w && g_noise);
  CONTRAD_ARG(P >= 1 && P <= (1ll << 40) && K >= 1 && K <= 65536);
  const bool vec = (K % 4 == 0) && (((uintptr_t)g_pre & 15) == 0);
  const int per = vec ? K / 4 : K;
  int lpshift = 0;
  while ((1 << lpshift) < per && lpshift < 6) ++lpshift;
  const long long blocks = cdivll(P << lpshift, PROJ_THREADS);
  CONTRAD_ARG(blocks <= 0x7fffffffll);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(noise_grad_kernel<true>, dim3((unsigned)blocks), dim3(PROJ_THREADS), 0, st, g_pre, noise_w, g_noise, P, K, lpshift);
  else
    hipLaunchKernelGGL(noise_grad_kernel<false>, dim3((unsigned)blocks), dim3(PROJ_THREADS), 0, st, g_pre, noise_w, g_noise, P, K, lpshift);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_proj_noise_reg(const float* map, float* reg, float* g_acc, float scale, float* scratch, long long scratch_floats,
                                      int N, int R, contrad_stream_t stream) {
  CONTRAD_ARG(map && reg && g_acc && scratch);
  CONTRAD_ARG(N >= 1 && N <= 65535 && R >= 4 && R <= 1024 && pow2(R));
  CONTRAD_ARG(((uintptr_t)map & 15) == 0 && ((uintptr_t)scratch & 15) == 0);
  CONTRAD_ARG(scale == scale && scale - scale == 0.f);                // finite
  CONTRAD_ARG(g_acc != map);
  const RegPlan p = reg_plan(R);
  const long long need = (long long)N * (p.pyr + (long long)p.J * p.nblk0 * 2 + (long long)p.J * 2);
  CONTRAD_ARG(scratch_floats >= need);
  float* pyr = scratch;
  float* part = pyr + (long long)N * p.pyr;
  float* coef = part + (long long)N * p.J * p.nblk0 * 2;
  RegOff off;
  for (int j = 0; j < REG_MAX_LEVELS; ++j) off.v[j] = p.off[j];
  hipStream_t st = (hipStream_t)stream;
  if (p.J > 1) {
    const int T = R < REG_TILE ? R : REG_TILE, tiles = R / T;
    hipLaunchKernelGGL(reg_pyramid_kernel, dim3((unsigned)(tiles * tiles), (unsigned)N), dim3(PROJ_THREADS), 0, st, map, pyr, off, p.pyr, R,
                       T, p.J);
    CONTRAD_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(reg_products_kernel, dim3((unsigned)p.nblk0, (unsigned)p.J, (unsigned)N), dim3(PROJ_THREADS), 0, st, map, pyr, part, off,
                     p.pyr, R, p.J, p.nblk0);
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(reg_finish_kernel, dim3((unsigned)N), dim3(64), 0, st, part, coef, reg, R, p.J, p.nblk0);
  CONTRAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(reg_grad_kernel, dim3((unsigned)cdiv(R * R, PROJ_THREADS), (unsigned)N), dim3(PROJ_THREADS), 0, st, map, pyr, coef,
                     g_acc, off, p.pyr, R, p.J, scale);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}

extern "C" int contrad_proj_noise_normalize(float* map, int N, int R, contrad_stream_t stream) {
  CONTRAD_ARG(map);
  CONTRAD_ARG(N >= 1 && R >= 4 && R <= 1024 && pow2(R));
  CONTRAD_ARG(((uintptr_t)map & 15) == 0);
  const int count = R * R;
  const int threads = count >= 65536 ? 1024 : PROJ_THREADS;
  hipLaunchKernelGGL(noise_normalize_kernel, dim3((unsigned)N), dim3(threads), 0, (hipStream_t)stream, map, count);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
