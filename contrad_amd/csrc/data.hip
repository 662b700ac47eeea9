// Real-image batches from a device-resident uint8 set (contrad_amd/data.py): ONE launch gathers B images by index, flips
// the marked ones, transposes NHWC -> NCHW and converts to ToTensor's floats,
//     dst[b, c, i, j] = (float) src[idx_b, i, (flip_b ? W-1-j : j), c] / 255.0f.
// The division is the correctly rounded fp32 one (this file is built without fast-math and calls __fdiv_rn): the pixels
// are bit-equal to x.float().div(255).  A multiply by 1/255 is not, for some of the 256 byte values.
//
// Lane mapping: a lane owns FOUR consecutive output columns of one row, in all three channel planes.  Its 12 source bytes
// are contiguous (a flipped row reads the same 12 bytes of the mirrored columns and reverses the four pixels in
// registers), and it writes one 16-byte store per plane.  Consecutive lanes own consecutive column quads, so a wave reads
// 768 contiguous bytes and writes 1 KiB contiguous per plane.
//   * aligned form (W % 4 == 0, dst 16-byte aligned, src 4-byte aligned): rows follow each other without a gap, item t of an
//     image is floats [4t, 4t+4) of each plane and bytes [12t, 12t+12) of the image; three dword loads, three 16-byte stores.
//   * general form (W % 4 != 0, an image stride H*W*3 off the 4-byte grid, base pointers off the grid): every row is split
//     as csrc/gp.hip splits its rows -- a scalar head up to the first 16-byte aligned address of the row in plane 0, quads
//     from there, a scalar tail.  A quad stores 16 bytes into every plane whose address is 16-byte aligned (plane 0 always;
//     all three when H*W % 4 == 0) and four floats otherwise; it loads three dwords when its 12 bytes start on the 4-byte
//     grid and 12 bytes otherwise.
// No atomics, no LDS: every output float is written once by one lane, two calls are bitwise equal.
// An index outside [0, n) (or NaN) is clamped to the nearest valid image, so no parameter block makes the kernel read
// outside src.
#include "common.h"
#include "../../include/contrad_hip.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_MAX_N = 1 << 24;       // indices travel as floats: every one up to 2^24 - 1 is exact

__device__ __forceinline__ int dg_index(float f, int n) {
  return f >= 0.f ? (int)fminf(f, (float)(n - 1)) : 0;        // NaN -> 0, +inf -> n - 1
}

__device__ __forceinline__ float dg_unit(unsigned v) { return __fdiv_rn((float)v, 255.0f); }

// the 12 bytes of four RGB pixels, as three little-endian dwords
struct DgQuad { unsigned w[3]; };

__device__ __forceinline__ DgQuad dg_load_dwords(const unsigned char* p) {
  const unsigned* q = reinterpret_cast<const unsigned*>(p);
  DgQuad r;
  r.w[0] = q[0]; r.w[1] = q[1]; r.w[2] = q[2];
  return r;
}

__device__ __forceinline__ DgQuad dg_load_bytes(const unsigned char* p) {
  DgQuad r;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    r.w[k] = (unsigned)p[4 * k] | ((unsigned)p[4 * k + 1] << 8) | ((unsigned)p[4 * k + 2] << 16) | ((unsigned)p[4 * k + 3] << 24);
  return r;
}

// channel c of the four pixels in OUTPUT order (flip: source pixel 3 - k feeds output column k)
__device__ __forceinline__ f32x4 dg_plane(const DgQuad& s, int c, bool flip) {
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int byte = 3 * k + c;                                // source pixel k, channel c
    const float v = dg_unit((s.w[byte >> 2] >> (8 * (byte & 3))) & 255u);
    o[k] = v;
  }
  if (flip) { const f32x4 r = {o[3], o[2], o[1], o[0]}; return r; }
  return o;
}

// grid (items of an image / 256, images): block row y makes images y, y + gridDim.y, ...
template <bool ALIGNED>
__global__ __launch_bounds__(DG_THREADS) void gather_u8_nchw_kernel(const unsigned char* __restrict__ src,
                                                                    const float* __restrict__ params,
                                                                    float* __restrict__ dst, int B, int n, int H, int W) {
  const int t = blockIdx.x * DG_THREADS + threadIdx.x;
  const size_t HW = (size_t)H * W;
  if (ALIGNED) {
    const int wq = W >> 2;                                     // quads of a row
    if (t >= H * wq) return;
    const int i = t / wq, q = t - i * wq;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
      const int id = dg_index(params[2 * b], n);
      const bool flip = params[2 * b + 1] != 0.f;
      const size_t pix = (size_t)i * W + (flip ? W - 4 - 4 * q : 4 * q);
      const DgQuad s = dg_load_dwords(src + ((size_t)id * HW + pix) * 3);
      float* d = dst + (size_t)b * 3 * HW + 4 * (size_t)t;
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(d + c * HW) = dg_plane(s, c, flip);
    }
    return;
  }
  const int slots = (W >> 2) + 2;                              // per row: the head, up to W / 4 quads, the tail
  if (t >= H * slots) return;
  const int i = t / slots, sl = t - i * slots;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int id = dg_index(params[2 * b], n);
    const bool flip = params[2 * b + 1] != 0.f;
    const unsigned char* srow = src + ((size_t)id * HW + (size_t)i * W) * 3;
    float* drow = dst + (size_t)b * 3 * HW + (size_t)i * W;    // plane 0; plane c is c * HW floats further
    const int off = (int)(((uintptr_t)drow >> 2) & 3);         // floats behind a 16-byte aligned address
    const int head = min(W, (4 - off) & 3);
    const int nvec = (W - head) >> 2;
    const int tail0 = head + 4 * nvec;
    if (sl >= 1 && sl <= nvec) {
      const int j0 = head + 4 * (sl - 1);
      const unsigned char* sp = srow + (size_t)(flip ? W - 4 - j0 : j0) * 3;
      const DgQuad s = (((uintptr_t)sp & 3) == 0) ? dg_load_dwords(sp) : dg_load_bytes(sp);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* p = drow + c * HW + j0;
        const f32x4 v = dg_plane(s, c, flip);
        if (((uintptr_t)p & 15) == 0) {
          *reinterpret_cast<f32x4*>(p) = v;
        } else {
          p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
        }
      }
    } else if (sl == 0 || sl == nvec + 1) {
      const int lo = sl == 0 ? 0 : tail0, hi = sl == 0 ? head : W;
      for (int j = lo; j < hi; ++j) {
        const unsigned char* sp = srow + (size_t)(flip ? W - 1 - j : j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) drow[c * HW + j] = dg_unit(sp[c]);
      }
    }
  }
}

}  // namespace

extern "C" int contrad_gather_u8_nchw(const unsigned char* src, const float* params, float* dst, int B, int n, int H, int W,
                                      contrad_stream_t stream) {
  CONTRAD_ARG(src && params && dst);
  CONTRAD_ARG(B > 0 && n > 0 && n <= DG_MAX_N && H > 0 && W > 0);
  CONTRAD_ARG((long long)H * ((W >> 2) + 2) < (1ll << 31) - DG_THREADS);     // items of an image index with int
  CONTRAD_ARG(((uintptr_t)params & 3) == 0 && ((uintptr_t)dst & 3) == 0);
  const bool aligned = (W & 3) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)src & 3) == 0;
  const long long items = aligned ? (long long)H * (W >> 2) : (long long)H * ((W >> 2) + 2);
  const dim3 grid((unsigned)cdivll(items, DG_THREADS), (unsigned)(B < 65535 ? B : 65535));
  if (aligned)
    hipLaunchKernelGGL(gather_u8_nchw_kernel<true>, grid, dim3(DG_THREADS), 0, (hipStream_t)stream, src, params, dst, B, n, H, W);
  else
    hipLaunchKernelGGL(gather_u8_nchw_kernel<false>, grid, dim3(DG_THREADS), 0, (hipStream_t)stream, src, params, dst, B, n, H,
                       W);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
