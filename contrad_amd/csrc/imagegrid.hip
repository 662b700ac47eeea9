// Images for the host (contrad_amd/sample.py, contrad_amd/evaluate/gan.py): the inverse direction of csrc/data.hip.  ONE
// launch lays n float NCHW images (3 channels) out on a uint8 HWC canvas as torchvision's make_grid(images, nrow,
// padding = pad, pad_value) does and quantises every canvas value as save_image does:
//     canvas [ymaps * (H + pad) + pad, xmaps * (W + pad) + pad, 3],  ymaps = ceil(n / xmaps);
//     image k has its top-left pixel at (pad + (k / xmaps) * (H + pad), pad + (k % xmaps) * (W + pad));
//     everything else -- the frame, the gutters, the empty cells of a partly filled last row -- holds pad_value;
//     byte = trunc(clamp(v * 255 + 0.5, 0, 255)).
// The multiply and the add are rounded separately (__fmul_rn / __fadd_rn: no contraction into an FMA, whatever the compile
// flags), so the bytes equal v.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8) on the CPU.  NaN is written as 0 (the
// clamp is fminf(fmaxf(., 0), 255), which drops a NaN operand; torch leaves this case to the platform's float -> integer
// conversion), +inf as 255, -inf as 0.  pad_value goes through the same quantisation as a pixel.
// With pad = 0 and xmaps = 1 the canvas is the uint8 [n, H, W, 3] batch: the same kernel serves the sample writer.
//
// Lane mapping (output-centred, as data.hip): a lane owns FOUR consecutive canvas pixels in linear (row-major) order, i.e.
// the 12 bytes at byte 12 t of dst: three dword stores, always aligned when dst is 4-byte aligned, and a wave writes 768
// contiguous bytes.  The four pixels may straddle a canvas row, a gutter or two images, so the lane decides per pixel
// whether it is image or padding (one division for the lane's first pixel, then increments with a row wrap) and reads the
// three plane floats of an image pixel: consecutive lanes read consecutive 16-byte pieces of an image row in each plane,
// broken only where a row of a cell ends.  src needs 4-byte alignment only (scalar float loads).  When the pixel count is no
// multiple of 4, one more lane writes the last 1-3 pixels byte by byte.
// No memset, no atomics, no LDS: every output byte is written once by one lane, two calls are bitwise equal.
#include "common.h"
#include "../../include/contrad_hip.h"

namespace {

constexpr int IG_THREADS = 256;

__device__ __forceinline__ unsigned ig_quant(float v) {
  const float s = __fadd_rn(__fmul_rn(v, 255.0f), 0.5f);
  return (unsigned)fminf(fmaxf(s, 0.0f), 255.0f);             // NaN -> 0 (fmaxf returns the other operand)
}

struct IgGeom {
  int n, H, W, xmaps, pad, CW;
  long long pixels;                                            // canvas pixels
};

// the three bytes (r | g << 8 | b << 16) of canvas pixel (y, x)
__device__ __forceinline__ unsigned ig_pixel(const float* __restrict__ src, const IgGeom& g, int y, int x, unsigned padq) {
  const int gy = y - g.pad, gx = x - g.pad;
  if (gy < 0 || gx < 0) return padq;
  const int ch = g.H + g.pad, cw = g.W + g.pad;
  const int cy = gy / ch, iy = gy - cy * ch;
  const int cx = gx / cw, ix = gx - cx * cw;
  if (iy >= g.H || ix >= g.W) return padq;
  const long long k = (long long)cy * g.xmaps + cx;            // cx < xmaps, cy < ymaps by the canvas extents
  if (k >= g.n) return padq;
  const size_t HW = (size_t)g.H * g.W;
  const float* p = src + (size_t)k * 3 * HW + (size_t)iy * g.W + ix;
  return ig_quant(p[0]) | (ig_quant(p[HW]) << 8) | (ig_quant(p[2 * HW]) << 16);
}

__global__ __launch_bounds__(IG_THREADS) void image_grid_u8_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst,
                                                                   IgGeom g, float pad_value) {
  const long long t = (long long)blockIdx.x * IG_THREADS + threadIdx.x;
  const long long quads = g.pixels >> 2;
  if (t > quads) return;
  const unsigned pq = ig_quant(pad_value);
  const unsigned padq = pq | (pq << 8) | (pq << 16);
  const long long p0 = 4 * t;
  int y = (int)(p0 / g.CW), x = (int)(p0 - (long long)y * g.CW);
  if (t < quads) {
    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[k] = ig_pixel(src, g, y, x, padq);
      if (++x == g.CW) { x = 0; ++y; }
    }
    unsigned* d = reinterpret_cast<unsigned*>(dst + 12 * (size_t)t);
    d[0] = px[0] | (px[1] << 24);
    d[1] = (px[1] >> 8) | (px[2] << 16);
    d[2] = (px[2] >> 16) | (px[3] << 8);
    return;
  }
  const int rest = (int)(g.pixels & 3);                         // t == quads: the scalar tail (nothing when rest == 0)
  for (int k = 0; k < rest; ++k) {
    const unsigned v = ig_pixel(src, g, y, x, padq);
    unsigned char* d = dst + 3 * (size_t)(p0 + k);
    d[0] = (unsigned char)(v & 255u); d[1] = (unsigned char)((v >> 8) & 255u); d[2] = (unsigned char)(v >> 16);
    if (++x == g.CW) { x = 0; ++y; }
  }
}

}  // namespace

extern "C" int contrad_image_grid_u8(const float* src, unsigned char* dst, int n, int H, int W, int xmaps, int pad,
                                     float pad_value, contrad_stream_t stream) {
  CONTRAD_ARG(src && dst);
  CONTRAD_ARG(n > 0 && H > 0 && W > 0 && xmaps > 0 && pad >= 0);
  CONTRAD_ARG(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0);
  const long long ymaps = cdivll(n, xmaps);
  const long long CH = ymaps * ((long long)H + pad) + pad, CW = (long long)xmaps * ((long long)W + pad) + pad;
  CONTRAD_ARG(CH < (1ll << 31) && CW < (1ll << 31));                          // canvas coordinates index with int
  CONTRAD_ARG((long long)H * W < (1ll << 31));
  const long long pixels = CH * CW;
  const long long blocks = cdivll((pixels >> 2) + 1, IG_THREADS);             // + 1: the tail lane
  CONTRAD_ARG(blocks < (1ll << 31));
  IgGeom g;
  g.n = n; g.H = H; g.W = W; g.xmaps = xmaps; g.pad = pad; g.CW = (int)CW; g.pixels = pixels;
  hipLaunchKernelGGL(image_grid_u8_kernel, dim3((unsigned)blocks), dim3(IG_THREADS), 0, (hipStream_t)stream, src, dst, g,
                     pad_value);
  CONTRAD_CHECK_LAUNCH();
  return 0;
}
