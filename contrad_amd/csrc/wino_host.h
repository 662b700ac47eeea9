// Host layer of the Winograd kernels (wino.h, wino44.h, wino44n.h, wino22.h, wino23.h): which shapes each family runs, when the
// plan sends a layer there, its launch arguments and grid, and the launches.  Included by igemm.hip after the five kernel headers,
// inside its anonymous namespace.  Every decision the families share is written once at the top; a family is a struct with its
// shape rule (ok), geometry (args), plan rule (planned) and kernel-instance choice (launch), and one row of WINO_FAMILIES.

constexpr int WINO_CUS = 256;      // one persistent block per CU of the MI355X

// The two sides of a layer as a forward / data-gradient kernel sees them: the data gradient reads gy and writes dx.
struct Sides { int cin, cout, ldi, ldo; };
inline Sides sides(const contrad_conv_desc* d, int mode) {
  if (mode == MODE_FWD) return {d->C, d->K, d->ldx, d->ldy};
  return {d->K, d->C, d->ldy, d->ldx};
}

// Does a launch of `items` whole-CU items fill the chip well enough?  A single partial round from min_items, else a last round
// that is not mostly empty (rounds x CUs <= num / den x items).
inline bool fills_chip(long long items, long long min_items, int num, int den) {
  if (items < WINO_CUS) return items >= min_items;
  return cdivll(items, WINO_CUS) * WINO_CUS * den <= items * num;
}

// The persistent grid: blocks go to the XCDs round-robin and every XCD walks its own items, so no XCD needs more blocks than the
// fullest one has items.
inline int persistent_grid(int xcd_items) { return 8 * std::min(WINO_CUS / 8, xcd_items); }

// An item is one block of tiles x one block of output channels.  F::items(a, xcds) counts those of the fullest of `xcds` XCDs when
// the tile blocks are dealt to them in turn: with 1 the items of the launch, with 8 what sizes the grid.
template <class F>
int family_grid(const contrad_conv_desc* d, int mode) { return persistent_grid((int)F::items(F::args(d, mode), 8)); }

// The forward / data-gradient launch of a family.  U is the workspace, filled here by the family's own filter kernel, or the
// caller's prepared filter Uprep.
template <class F, int MODE>
int launch_family(const contrad_conv_desc* d, const float* in, const float* wp, const float* bias, const float* ref, float* out,
                  float slope, float gain, float* U, hipStream_t stream, const float* Uprep) {
  typename F::Args a = F::args(d, MODE);
  a.x = in; a.U = Uprep ? Uprep : U; a.y = out; a.bias = bias; a.ref = ref; a.slope = slope; a.gain = gain;
  const int quads = F::PHASES * (a.Cin / 4) * a.Cout;
  if (!Uprep) hipLaunchKernelGGL(F::template filter_kernel<MODE>, dim3(cdiv(quads, 256)), dim3(256), 0, stream, wp, U, d->C, d->K, d->ldw);
  CONTRAD_CHECK_LAUNCH();
  return F::template launch<MODE>(a, persistent_grid((int)F::items(a, 8)), stream);
}

// ---------------- Winograd F(2x2, 3x3) path (wino.h): 3x3 stride-1 pad-1 layers, forward and data gradient ----------------
struct Wino {
  using Args = wino::Args;
  static constexpr int PHASES = 1;
  template <int MODE> static constexpr auto filter_kernel = wino::wino_filter_kernel<MODE>;

  // Can the shape run on wino_kernel<mode> at all?  (input channels % 16, output channels % 64, power-of-two maps >= 4)
  static bool ok(const contrad_conv_desc* d, int mode) {
    if (mode != MODE_FWD && mode != MODE_DGRAD) return false;
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1) return false;
    if (d->H < 4 || d->W < 4 || (d->H & (d->H - 1)) || (d->W & (d->W - 1))) return false;
    const Sides s = sides(d, mode);
    if ((s.cin & 15) || (s.cout & 63) || (s.ldi & 3) || (d->ldw & 3)) return false;
    const int th = std::min(8, d->H / 2), tw = std::min(8, d->W / 2);
    const long long nimg = 64 / (th * tw);
    if (nimg > 16) return false;
    const long long lim = 1ll << 31;
    if (nimg * d->H * d->W * std::max(s.ldi, s.ldo) * 4 >= lim) return false;     // block-relative byte offsets
    if (16ll * s.cin * s.cout * 4 >= lim) return false;
    return true;
  }

  static Args args(const contrad_conv_desc* d, int mode) {
    Args a{};
    const Sides s = sides(d, mode);
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.Cin = s.cin; a.Cout = s.cout; a.ldi = s.ldi; a.ldo = s.ldo;
    a.TH = std::min(8, d->H / 2); a.TW = std::min(8, d->W / 2);
    a.sh_tw = __builtin_ctz(a.TW); a.sh_thw = __builtin_ctz(a.TH * a.TW);
    a.NIMG = 64 / (a.TH * a.TW);
    a.PH = d->H / (2 * a.TH); a.PW = d->W / (2 * a.TW);
    a.NP = cdiv(d->N, a.NIMG) * a.PH * a.PW;
    a.NKB = a.Cout / 64;
    // raw box: with the halo (pixels outside the image load as zeros) when the image has several patches along the axis,
    // else the image itself (the halo reads the zero pixel)
    a.BH = a.PH > 1 ? 2 * a.TH + 2 : d->H; a.r_org = a.PH > 1 ? -1 : 0;
    a.BW = a.PW > 1 ? 2 * a.TW + 2 : d->W; a.c_org = a.PW > 1 ? -1 : 0;
    return a;
  }
  static long long items(const Args& a, int xcds) { return (long long)cdiv(a.NP, xcds) * a.NKB; }

  // Does the plan send the layer there?  A block is a whole CU and an item (64 tiles x 64 couts x all channels) its unit of
  // work: the launch needs about a round of items, and the last round must not be mostly empty.  (Behind Wino44 in the table:
  // F(4x4, 3x3) takes the launch when it is planned.)
  static bool planned(const contrad_conv_desc* d, int mode) {
    static const bool enabled = contrad_dev_on("CONTRAD_WINO");
    if (!enabled || !ok(d, mode)) return false;
    // (a single partial round: from 150 items.  Per-rank batches of the headline config on one GPU, profiles/r06_ab_plan_thresholds.txt:
    // 200 / 150 / 90 items -> 3.12 / 2.82 / 2.89 ms per step at batch 64, 4.39 / 4.25 / 4.24 at batch 128)
    static const long long min_items = contrad_dev_ll("CONTRAD_WINO_MIN_ITEMS", 150ll);
    return fills_chip(items(args(d, mode), 1), min_items, 14, 10);
  }

  template <int MODE>
  static int launch(const Args& a, int grid, hipStream_t stream) {
    return launch_large_lds<wino::wino_kernel<MODE>>(dim3(grid), 512, wino::LDS_DWORDS * 4, stream, a);
  }
};

// ---------------- Winograd F(4x4, 3x3) path (wino44.h): the same layers as wino.h on maps of 8x8 and larger ----------------
// (input channels % 32, output channels % 64 -- or an odd multiple of 32: wino44n.h --, power-of-two maps >= 8; 2.25 multiply-adds per
// output instead of 4)
struct Wino44 {
  using Args = wino44::Args;
  static constexpr int PHASES = 1;
  template <int MODE> static constexpr auto filter_kernel = wino44::wino44_filter_kernel<MODE>;

  static bool ok(const contrad_conv_desc* d, int mode) {
    if (mode != MODE_FWD && mode != MODE_DGRAD) return false;
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1) return false;
    // (4x4 maps: wino44n_kernel only -- a tile is an image, 32 images per item)
    if (d->H < 4 || d->W < 4 || (d->H & (d->H - 1)) || (d->W & (d->W - 1)) || (d->W < 32 ? d->H != d->W : d->H < 16)) return false;
    const Sides s = sides(d, mode);
    // (output channels: whole 64-wide blocks -- wino44_kernel -- or an odd number of 32-wide ones -- wino44n_kernel, wino44n.h)
    if ((s.cin & 31) || (s.cout & 31) || (s.ldi & 3) || (d->ldw & 3)) return false;
    const long long lim = 1ll << 31;
    const long long nimg = d->W >= 32 ? 1 : d->W == 16 ? 2 : d->W == 8 ? 8 : 32;
    if (nimg * d->H * d->W * std::max(s.ldi, s.ldo) * 4 >= lim) return false;     // block-relative byte offsets
    if (36ll * s.cin * s.cout * 4 >= lim) return false;
    return true;
  }

  // A single round from 230 items, else a last round that is not mostly empty (rounds x CUs <= 1.4 x items).
  static bool round_ok(long long items) {
    static const long long min_items = contrad_dev_ll("CONTRAD_WINO44_MIN_ITEMS", 230ll);
    return fills_chip(items, min_items, 14, 10);
  }

  // patches (32 tiles each) of a launch: images / images per item x patches per image
  static long long patches(const contrad_conv_desc* d) {
    const int TW = std::min(8, d->W / 4), TH = std::min(4, d->H / 4);
    return (long long)cdiv(d->N, 32 / (TH * TW)) * (d->H / (4 * TH)) * (d->W / (4 * TW));
  }

  // wino44n_kernel (items of 32 tiles x 32 couts) instead of wino44_kernel (x 64): output channels that are not whole 64-wide blocks;
  // the 4x4 maps (1536 images x 512 couts: 768 items = three full rounds where 64-wide blocks give one and a half); and launches
  // whose 64-wide items do not fill the chip while twice as many half items do (192 images of 8 x 8 x 512: 192 -> 384 items, 0.30 ->
  // 0.24 ms; of 16 x 16 x 128: 0.095 -> 0.079 ms -- with enough items the 64-wide blocks are 10 - 25 % faster: one exchange and one
  // transform of V per 64 couts instead of per 32, profiles/r06_ab_wino44n_plan.txt)
  static bool n32(const contrad_conv_desc* d, int mode) {
    static const bool all = contrad_dev_off_by_default("CONTRAD_WINO44N_ALL");      // (dev: every shape on it)
    static const bool fill = contrad_dev_on("CONTRAD_WINO44N_FILL");  // (dev: the third rule off)
    const int cout = sides(d, mode).cout;
    if ((cout & 63) != 0 || d->W == 4 || all) return true;
    const long long items64 = patches(d) * (cout / 64);
    return fill && !round_ok(items64) && round_ok(2 * items64);
  }

  static Args args(const contrad_conv_desc* d, int mode) {
    Args a{};
    const Sides s = sides(d, mode);
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.Cin = s.cin; a.Cout = s.cout; a.ldi = s.ldi; a.ldo = s.ldo;
    a.TW = std::min(8, d->W / 4); a.TH = std::min(4, d->H / 4);      // 4x4-pixel tiles per image part of an item: 4 x 8, 4 x 4 (16x16 maps), 2 x 2 (8x8), 1 (4x4)
    a.sh_tw = __builtin_ctz(a.TW); a.sh_thw = __builtin_ctz(a.TH * a.TW);
    a.NIMG = 32 / (a.TH * a.TW);
    a.PH = d->H / (4 * a.TH); a.PW = d->W / (4 * a.TW);
    a.NP = cdiv(d->N, a.NIMG) * a.PH * a.PW;
    a.n32 = n32(d, mode) ? 1 : 0;
    a.NKB = a.n32 ? a.Cout / 32 : a.Cout / 64;      // 32-wide cout blocks: the items of wino44n_kernel
    a.BH = 4 * a.TH + 2; a.BW = 4 * a.TW + 2;       // raw box: always with the halo
    return a;
  }
  static long long items(const Args& a, int xcds) { return (long long)cdiv(a.NP, xcds) * a.NKB; }

  // An item is 512 output pixels x 64 (32) couts x all channels on a whole CU: twice wino.h's.  The plan takes F(4x4, 3x3) when the
  // launch has a full round of them and its last round is not mostly empty; else the layer falls through to Wino::planned.
  static bool planned(const contrad_conv_desc* d, int mode) {
    static const bool enabled = contrad_dev_on("CONTRAD_WINO44");
    static const bool enabled2 = contrad_dev_on("CONTRAD_WINO");
    if (!enabled || !enabled2 || !ok(d, mode)) return false;
    static const bool enabled_n = contrad_dev_on("CONTRAD_WINO44N");
    if (!enabled_n && n32(d, mode)) return false;       // (32-wide cout blocks: wino44n.h)
    return round_ok(items(args(d, mode), 1));
  }

  // raw boxes 34 / 18 / 10 pixels wide (maps from 32 / of 16 / of 8), and 6 (4x4 maps: wino44n_kernel only)
  template <int MODE>
  static int launch(const Args& a, int grid, hipStream_t stream) {
    constexpr size_t lds = wino44::LDS_DWORDS * 4;
    if (a.n32)
      return a.BW == 34   ? launch_large_lds<wino44n::wino44n_kernel<MODE, 34>>(dim3(grid), 512, lds, stream, a)
             : a.BW == 18 ? launch_large_lds<wino44n::wino44n_kernel<MODE, 18>>(dim3(grid), 512, lds, stream, a)
             : a.BW == 10 ? launch_large_lds<wino44n::wino44n_kernel<MODE, 10>>(dim3(grid), 512, lds, stream, a)
                          : launch_large_lds<wino44n::wino44n_kernel<MODE, 6>>(dim3(grid), 512, lds, stream, a);
    return a.BW == 34   ? launch_large_lds<wino44::wino44_kernel<MODE, 34>>(dim3(grid), 512, lds, stream, a)
           : a.BW == 18 ? launch_large_lds<wino44::wino44_kernel<MODE, 18>>(dim3(grid), 512, lds, stream, a)
                        : launch_large_lds<wino44::wino44_kernel<MODE, 10>>(dim3(grid), 512, lds, stream, a);
  }
};

// ---------------- Winograd F(2x2, 2x2) path (wino22.h): 4x4 stride-2 pad-1 layers, forward and data gradient ----------------
struct Wino22 {
  using Args = wino22::Args;
  static constexpr int PHASES = 4;
  template <int MODE> static constexpr auto filter_kernel = wino22::wino22_filter_kernel<MODE>;

  static bool ok(const contrad_conv_desc* d, int mode) {
    if (mode != MODE_FWD && mode != MODE_DGRAD) return false;
    if (d->KH != 4 || d->KW != 4 || d->stride != 2 || d->pad != 1) return false;
    if ((d->H & 1) || (d->W & 1) || d->Ho * 2 != d->H || d->Wo * 2 != d->W) return false;
    auto grid_ok = [](int g) { return g == 4 || g == 8 || g == 16; };
    if (!grid_ok(d->Ho) || !grid_ok(d->Wo)) return false;
    const Sides s = sides(d, mode);
    if ((s.cin & (mode == MODE_FWD ? 7 : 15)) || (s.cout & 63) || (s.ldi & 3) || (d->ldw & 3)) return false;
    const long long nimg = wino22::TB / ((d->Ho / 2) * (d->Wo / 2));
    const long long lim = 1ll << 31;
    if (nimg * d->H * d->W * std::max(d->ldx, d->ldy) * 4 >= lim) return false;
    if (4ll * 9 * s.cin * s.cout * 4 >= lim) return false;
    return true;
  }

  static Args args(const contrad_conv_desc* d, int mode) {
    Args a{};
    const bool dg = mode == MODE_DGRAD;
    const Sides s = sides(d, mode);
    a.N = d->N; a.dgrad = dg ? 1 : 0;
    a.Hi = dg ? d->Ho : d->H; a.Wi = dg ? d->Wo : d->W;
    a.Hout = dg ? d->H : d->Ho; a.Wout = dg ? d->W : d->Wo;
    a.Cin = s.cin; a.Cout = s.cout; a.ldi = s.ldi; a.ldo = s.ldo;
    a.GH = d->Ho; a.GW = d->Wo;
    const int tw = a.GW / 2, thw = (a.GH / 2) * tw;
    a.sh_tw = __builtin_ctz(tw); a.sh_thw = __builtin_ctz(thw);
    a.NIMG = wino22::TB / thw;
    a.NTB = cdiv(d->N, a.NIMG);
    a.NKB = a.Cout / 64;
    return a;
  }
  static long long items(const Args& a, int xcds) { return (long long)cdiv(a.NTB, xcds) * a.NKB * (a.dgrad ? 4 : 1); }      // (data gradient: one item per dx phase)

  static bool planned(const contrad_conv_desc* d, int mode) {
    static const bool enabled = contrad_dev_on("CONTRAD_WINO22");
    if (!enabled || !ok(d, mode)) return false;
    // (1.78x fewer multiply-adds, not 2.25x: a last round that is a quarter empty already loses to the direct kernels -- forward of
    // 256 -> 512 channels at 1536 images, 384 items: 0.622 ms against 0.558, profiles/r06_ab_wino22_layers.txt)
    static const long long min_items = contrad_dev_ll("CONTRAD_WINO22_MIN_ITEMS", 150ll);
    return fills_chip(items(args(d, mode), 1), min_items, 125, 100);
  }

  template <int MODE>
  static int launch(const Args& a, int grid, hipStream_t stream) {
    constexpr size_t lds = wino22::LDS_DWORDS * 4;
    const int nraw = cdiv(2 * a.NIMG * (a.GH + 1) * (a.GW + 1), 256);      // raw box pieces (pixel x k-quad) per mover thread and chunk
    if (nraw <= 5) return launch_large_lds<wino22::wino22_kernel<MODE, 5>>(dim3(grid), 512, lds, stream, a);
    if (nraw == 6) return launch_large_lds<wino22::wino22_kernel<MODE, 6>>(dim3(grid), 512, lds, stream, a);
    return launch_large_lds<wino22::wino22_kernel<MODE, 7>>(dim3(grid), 512, lds, stream, a);
  }
};

// ---------------- F(2x2, 2x2) on the phases of the 3x3 stride-2 pad-0 layers (wino23.h): StyleGAN2's blurred conv2, forward ----------------
// (input (2 Ho + 1) x (2 Wo + 1), power-of-two output grids >= 4, input channels % 16, output channels % 64; 25 of the dense
// layer's 36 multiply-adds)
struct Wino23 {
  using Args = wino23::Args;
  static constexpr int PHASES = 4;
  template <int MODE> static constexpr auto filter_kernel = wino23::wino23_filter_kernel;      // (forward only)

  static bool ok(const contrad_conv_desc* d, int mode) {
    if (mode != MODE_FWD) return false;
    if (d->KH != 3 || d->KW != 3 || d->stride != 2 || d->pad != 0) return false;
    if (d->H != 2 * d->Ho + 1 || d->W != 2 * d->Wo + 1) return false;
    if (d->Ho < 4 || d->Wo < 4 || (d->Ho & (d->Ho - 1)) || (d->Wo & (d->Wo - 1))) return false;
    if (d->Wo >= 32 ? d->Ho < 16 : d->Ho != d->Wo) return false;
    if ((d->C & 15) || (d->K & 63) || (d->ldx & 3) || (d->ldw & 3)) return false;
    const long long nimg = d->Wo >= 32 ? 1 : 128 / ((d->Ho / 2) * (d->Wo / 2));
    const long long lim = 1ll << 31;
    if (nimg * d->H * d->W * std::max(d->ldx, d->ldy) * 4 >= lim) return false;
    if (4ll * 9 * d->C * d->K * 4 >= lim) return false;
    return true;
  }

  static Args args(const contrad_conv_desc* d, int /*mode: forward*/) {
    Args a{};
    a.N = d->N; a.Hi = d->H; a.Wi = d->W; a.GH = d->Ho; a.GW = d->Wo;
    a.Cin = d->C; a.Cout = d->K; a.ldi = d->ldx; a.ldo = d->ldy;
    a.TW = d->Wo >= 32 ? 16 : d->Wo / 2; a.TH = d->Wo >= 32 ? 8 : d->Ho / 2;      // patches of 8 x 16 tiles, or whole images
    a.sh_tw = __builtin_ctz(a.TW); a.sh_thw = __builtin_ctz(a.TH * a.TW);
    a.NIMG = wino23::TB / (a.TH * a.TW);
    a.PH = d->Ho / (2 * a.TH); a.PW = d->Wo / (2 * a.TW);
    a.NP = cdiv(d->N, a.NIMG) * a.PH * a.PW;
    a.NKB = a.Cout / 64;
    return a;
  }
  static long long items(const Args& a, int xcds) { return (long long)cdiv(a.NP, xcds) * a.NKB; }

  static bool planned(const contrad_conv_desc* d, int mode) {
    static const bool enabled = contrad_dev_on("CONTRAD_WINO23");
    if (!enabled || !ok(d, mode)) return false;
    return fills_chip(items(args(d, mode), 1), 230, 14, 10);
  }

  template <int MODE>
  static int launch(const Args& a, int grid, hipStream_t stream) {
    constexpr size_t lds = wino23::LDS_DWORDS * 4;
    const int nraw = cdiv(2 * a.NIMG * (2 * a.TH + 1) * (2 * a.TW + 1), 256);
    if (nraw <= 5) return launch_large_lds<wino23::wino23_kernel<5>>(dim3(grid), 512, lds, stream, a);
    if (nraw == 6) return launch_large_lds<wino23::wino23_kernel<6>>(dim3(grid), 512, lds, stream, a);
    return launch_large_lds<wino23::wino23_kernel<7>>(dim3(grid), 512, lds, stream, a);
  }
};

// ---------------- the table: one row per transformed-filter kind, in the order conv_route tries them ----------------
// The kind of the filter U a family reads is the family's contrad_conv2d_path number (9 serves 11, the 32-wide blocks of
// wino44n.h, too).
enum { FILTER_WINO = 7, FILTER_WINO22 = 8, FILTER_WINO44 = 9, FILTER_WINO23 = 10 };

using WinoLaunch = int (*)(const contrad_conv_desc*, const float* in, const float* wp, const float* bias, const float* ref,
                           float* out, float slope, float gain, float* U, hipStream_t, const float* Uprep);
struct WinoFamily {
  int kind;                 // FILTER_*
  int points;               // transform points per filter: its bytes are the workspace a call needs
  int phases;               // filter-transform threads per (four input channels x one output channel)
  double executed;          // multiply-adds issued per nominal multiply-add
  bool (*ok)(const contrad_conv_desc*, int mode);
  bool (*planned)(const contrad_conv_desc*, int mode);
  int (*grid)(const contrad_conv_desc*, int mode);
  WinoLaunch launch[2];     // [MODE_FWD], [MODE_DGRAD]; nullptr: the family has no such kernel
};
template <class F>
constexpr WinoFamily wino_row(int kind, int points, double executed, bool dgrad) {
  return {kind, points, F::PHASES, executed, F::ok, F::planned, family_grid<F>,
          {launch_family<F, MODE_FWD>, dgrad ? launch_family<F, MODE_DGRAD> : nullptr}};
}
const WinoFamily WINO_FAMILIES[] = {
    wino_row<Wino44>(FILTER_WINO44, 36, 0.25, true),        // 36 transform-domain multiply-adds per 4x4 tile instead of 144
    wino_row<Wino>(FILTER_WINO, 16, 4.0 / 9.0, true),       // 16 transform-domain multiply-adds per 2x2 tile instead of 36
    wino_row<Wino22>(FILTER_WINO22, 36, 9.0 / 16.0, true),  // four phases x 9 per 2x2 tile instead of 64
    wino_row<Wino23>(FILTER_WINO23, 36, 25.0 / 36.0, false) // 9 + 6 + 6 + 4 planes of the four phases per 2x2 tile instead of 36
};

inline const WinoFamily* wino_family(int kind) {
  for (const WinoFamily& f : WINO_FAMILIES)
    if (f.kind == kind) return &f;
  return nullptr;
}

// bytes of the transformed filter of a known kind
inline long long filter_bytes(int kind, const contrad_conv_desc* d) {
  return (long long)wino_family(kind)->points * d->C * d->K * (long long)sizeof(float);
}

// threads of a job's transform (one per four input channels x one output channel [x phase]); 0 = unknown kind / mode
inline long long filter_threads(int kind, int mode, int C, int K) {
  const WinoFamily* f = wino_family(kind);
  if (!f || (mode != MODE_FWD && mode != MODE_DGRAD) || !f->launch[mode]) return 0;
  contrad_conv_desc d{};
  d.C = C; d.K = K;
  const Sides s = sides(&d, mode);
  return f->phases * (long long)(s.cin / 4) * s.cout;
}

// Was `u` made for the path this call is about to take?  (host check: kind, mode, shape and the weight it was made from)
inline bool filter_fits(const contrad_filter_job* u, int kind, int mode, const contrad_conv_desc* d, const float* wp) {
  return u && u->U && u->kind == kind && u->mode == mode && u->C == d->C && u->K == d->K && u->ldw == d->ldw && u->wp == wp &&
         ((uintptr_t)u->U & 15) == 0;
}

// ---------------- weight gradients on the Winograd kernels: wino_wgrad_kernel (3x3 stride 1), wino22_wgrad_kernel (4x4 stride 2) ----------------
// A block owns one (row block, 64-wide K block) of the transformed gradient and a run of qps chunks of tiles; the runs' partial
// sums (POINTS x C x K each, bias partials behind them) are summed by wgrad_reduce_kernel in fixed order.
int launch_wgrad_reduce(const float* ws, float* dwp, int Kg, int K, int ldw, int slabs, const float* bias_ws, float* dbias,
                        hipStream_t stream);      // (igemm.hip)

// chunks per split: as many splits as fill the chip once, at most one per chunk
inline int wgrad_qps(int chunks, int out_blocks) {
  const int splits = std::max(1, std::min(chunks, WINO_CUS / out_blocks));
  return cdiv(chunks, splits);
}

struct WinoWgrad {      // C % 64, K % 64
  using Args = wino::WArgs;
  static constexpr int POINTS = 9;      // the 3x3 taps
  static constexpr auto kernel = wino::wino_wgrad_kernel;
  static constexpr size_t LDS_BYTES = wino::W_LDS_DWORDS * 4;
  static bool enabled() {
    static const bool on = contrad_dev_on("CONTRAD_WINO_WGRAD") && contrad_dev_on("CONTRAD_WINO");
    return on;
  }
  static bool ok(const contrad_conv_desc* d) {
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1) return false;
    if (d->H < 4 || d->W < 4 || (d->H & (d->H - 1)) || (d->W & (d->W - 1))) return false;
    if ((d->C & 63) || (d->K & 63) || (d->ldx & 3) || (d->ldy & 3)) return false;
    const long long lim = 1ll << 31;
    if (2ll * d->H * d->W * std::max(d->ldx, d->ldy) * 4 >= lim) return false;     // chunk-relative byte offsets (<= 2 images)
    return true;
  }
  static Args args(const contrad_conv_desc* d) {
    Args a{};
    a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->C; a.K = d->K; a.ldx = d->ldx; a.ldy = d->ldy;
    a.CTW = std::min(4, d->W / 2);
    a.CTH = std::min(8 / a.CTW, d->H / 2);
    a.CNIMG = 8 / (a.CTH * a.CTW);
    a.sh_ctw = __builtin_ctz(a.CTW); a.sh_cthw = __builtin_ctz(a.CTH * a.CTW);
    a.QH = d->H / (2 * a.CTH); a.QW = d->W / (2 * a.CTW);
    a.Q = cdiv(d->N, a.CNIMG) * a.QH * a.QW;
    a.CB = d->C / 64; a.KB = d->K / 64;
    a.qps = wgrad_qps(a.Q, a.CB * a.KB);
    a.BH = a.QH > 1 ? 2 * a.CTH + 2 : d->H; a.r_org = a.QH > 1 ? -1 : 0;
    a.BW = a.QW > 1 ? 2 * a.CTW + 2 : d->W; a.c_org = a.QW > 1 ? -1 : 0;
    return a;
  }
  static int row_blocks(const Args& a) { return a.CB; }
};

struct Wino22Wgrad {
  using Args = wino22::WArgs;
  static constexpr int POINTS = 16;     // the 4x4 taps
  static constexpr auto kernel = wino22::wino22_wgrad_kernel;
  static constexpr size_t LDS_BYTES = wino22::W_LDS_DWORDS * 4;
  static bool enabled() {
    static const bool on = contrad_dev_on("CONTRAD_WINO22_WGRAD") && contrad_dev_on("CONTRAD_WINO22");
    return on;
  }
  static bool ok(const contrad_conv_desc* d) {
    if (d->KH != 4 || d->KW != 4 || d->stride != 2 || d->pad != 1) return false;
    if (d->Ho * 2 != d->H || d->Wo * 2 != d->W) return false;
    auto grid_ok = [](int g) { return g == 4 || g == 8 || g == 16; };
    if (!grid_ok(d->Ho) || !grid_ok(d->Wo)) return false;
    if ((d->C != 64 && (d->C & 127)) || (d->K & 63) || (d->ldx & 3) || (d->ldy & 3)) return false;
    if (2ll * d->H * d->W * std::max(d->ldx, d->ldy) * 4 >= (1ll << 31)) return false;
    // the movers' raw pieces (box, image, pixel, channel quad) wrap once at most and stay inside a raw stage: a grid or channel
    // rule widened above must not reach the kernel with a box it has no room for
    const Args a = args(d);
    const int raw_items = (128 / a.CPB) * a.CNIMG * (2 * a.CTH + 1) * (2 * a.CTW + 1) * (a.CPB / 4);
    if (raw_items < 256 * wino22::W_NRAW_FULL || raw_items > 256 * wino22::W_NRAW || raw_items * 4 > wino22::W_RAWSZ) return false;
    return true;
  }
  static Args args(const contrad_conv_desc* d) {
    Args a{};
    a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->C; a.K = d->K; a.ldx = d->ldx; a.ldy = d->ldy; a.GH = d->Ho; a.GW = d->Wo;
    a.CTW = std::min(4, a.GW / 2);
    a.CTH = std::min(8 / a.CTW, a.GH / 2);
    a.CNIMG = 8 / (a.CTH * a.CTW);
    a.sh_ctw = __builtin_ctz(a.CTW); a.sh_cthw = __builtin_ctz(a.CTH * a.CTW);
    a.QH = a.GH / (2 * a.CTH); a.QW = a.GW / (2 * a.CTW);
    a.Q = cdiv(d->N, a.CNIMG) * a.QH * a.QW;
    a.RBN = 4 * d->C / 128; a.KB = d->K / 64;
    a.CPB = std::min(d->C, 128); a.sh_cpb = __builtin_ctz(a.CPB);
    a.qps = wgrad_qps(a.Q, a.RBN * a.KB);
    return a;
  }
  static int row_blocks(const Args& a) { return a.RBN; }
};

template <class G> int wgrad_splits(const typename G::Args& a) { return cdiv(a.Q, a.qps); }
template <class G> int wgrad_grid(const typename G::Args& a) { return G::row_blocks(a) * a.KB * wgrad_splits<G>(a); }

// planned when every block gets a contraction long enough to pay for its prologue and its epilogue (the transform back to the
// taps), and the blocks are one round that fills at least 0.7 of the chip
template <class G>
bool wgrad_planned(const contrad_conv_desc* d) {
  if (!G::enabled() || !G::ok(d)) return false;
  const typename G::Args a = G::args(d);
  const long long blocks = wgrad_grid<G>(a);
  static const int min_qps = contrad_dev_int("CONTRAD_WINO_MIN_QPS", 16);
  return a.qps >= min_qps && blocks * 10 >= WINO_CUS * 7 && blocks <= WINO_CUS;
}

template <class G>
long long wgrad_workspace_bytes(const contrad_conv_desc* d) {
  return (long long)wgrad_splits<G>(G::args(d)) * ((long long)G::POINTS * d->C + 1) * d->K * (long long)sizeof(float);
}

template <class G>
int launch_wgrad(const contrad_conv_desc* d, const float* x, const float* gy, float* dwp, float* dbias, float* workspace,
                 hipStream_t stream) {
  typename G::Args a = G::args(d);
  const int splits = wgrad_splits<G>(a);
  a.x = x; a.gy = gy; a.ws = workspace;
  a.bias_ws = dbias ? workspace + (size_t)splits * G::POINTS * d->C * d->K : nullptr;
  const int rc = launch_large_lds<G::kernel>(dim3(wgrad_grid<G>(a)), 512, G::LDS_BYTES, stream, a);
  return rc ? rc : launch_wgrad_reduce(workspace, dwp, G::POINTS * d->C, d->K, d->ldw, splits, a.bias_ws, dbias, stream);
}
