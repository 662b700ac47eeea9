"""The persistent item walk of the Winograd forward / data-gradient kernels (csrc/wino.h, wino44.h, wino44n.h, wino22.h,
wino23.h), restated in plain Python from the documented rules of csrc/wino_host.h, and the table of launches on which
tests/test_wino_walks_gpu.py checks it against float64.  No GPU, no library: tests/test_wino_walks_cpu.py compares the
restatement with the shipped library's plan queries and proves what the table covers.

The rule (three lines in every kernel): a launch has NP tile blocks ("patches": image groups x patches per image) and NSUB
items per tile block (cout blocks; x 4 output phases for the strided data gradient).  Tile blocks are dealt to the 8 XCDs in
turn; XCD x owns the list of L_x = ceil((NP - x) / 8) * NSUB items, item w of it being tile block (w // NSUB) * 8 + x, sub-item
w % NSUB.  Block b = (xcd b & 7, slot b >> 3) of a grid of 8 * nslots blocks walks w = slot, slot + nslots, ... < L_xcd.  The
host sizes the grid as 8 * min(32, L_0): a block walks a second item only when L_0 > 32.
"""
import collections

CUS = 256

# (path, mode, N, H, W, C, K, k, stride, pad, what): C / K are the layer's input / output channels in both modes (the data
# gradient reads gy with K channels and writes dx with C); H x W is the layer's input map.  Every operand has a leading
# dimension of its channel count + 4 (the slice [4, 4 + channels) of a wider buffer).
WALK_CASES = [
    # F(2x2,3x3), Cin = 16: two chunks per item -- the raw stream (three chunks ahead) is in the item after next
    (7, 0, 2987, 4, 4, 16, 192, 3, 1, 1, '16 images per item, ragged'),
    (7, 0, 747, 8, 8, 16, 192, 3, 1, 1, '4 images per item, ragged'),
    (7, 0, 187, 16, 16, 16, 192, 3, 1, 1, 'one image per item: the box is the image'),
    (7, 0, 47, 32, 32, 16, 192, 3, 1, 1, '2 x 2 patches per image: boxes with halo'),
    (7, 1, 2987, 4, 4, 192, 16, 3, 1, 1, ''),
    (7, 1, 747, 8, 8, 192, 16, 3, 1, 1, ''),
    # F(4x4,3x3), 64-wide items, Cin = 32: four chunks (two pairs) per item
    (9, 0, 1493, 8, 8, 32, 192, 3, 1, 1, '8 images per item, ragged'),
    (9, 0, 373, 16, 16, 32, 192, 3, 1, 1, '2 images per item, ragged'),
    (9, 0, 94, 32, 32, 32, 192, 3, 1, 1, 'two patches per image'),
    (9, 1, 1493, 8, 8, 192, 32, 3, 1, 1, ''),
    (9, 1, 373, 16, 16, 192, 32, 3, 1, 1, ''),
    # F(4x4,3x3), 32-wide items (three of them: an odd number of 32-wide cout blocks)
    (11, 0, 5977, 4, 4, 32, 96, 3, 1, 1, 'a tile is an image, 32 per item, ragged'),
    (11, 0, 1493, 8, 8, 32, 96, 3, 1, 1, ''),
    (11, 0, 373, 16, 16, 32, 96, 3, 1, 1, ''),
    (11, 0, 94, 32, 32, 32, 96, 3, 1, 1, ''),
    (11, 1, 5977, 4, 4, 96, 32, 3, 1, 1, ''),
    (11, 1, 373, 16, 16, 96, 32, 3, 1, 1, ''),
    # F(2x2,2x2) on the phases of the 4x4 stride-2 layers; forward Cin = 8: one chunk per input phase
    (8, 0, 6583, 8, 8, 8, 192, 4, 2, 1, '4 x 4 grid: 32 images per item, ragged'),
    (8, 0, 1645, 16, 16, 8, 192, 4, 2, 1, '8 x 8 grid: 8 images per item, ragged'),
    (8, 0, 411, 32, 32, 8, 192, 4, 2, 1, '16 x 16 grid: 2 images per item, ragged'),
    # ... data gradient: an item per (cout block, dx phase), 12 per tile block; gy has 16 channels: two chunks per item
    (8, 1, 1655, 8, 8, 192, 16, 4, 2, 1, ''),
    (8, 1, 413, 16, 16, 192, 16, 4, 2, 1, ''),
    (8, 1, 103, 32, 32, 192, 16, 4, 2, 1, ''),
    # F(2x2,2x2) on the phases of the 3x3 stride-2 pad-0 layers, Cin = 16: one chunk pair per input phase
    (10, 0, 5977, 9, 9, 16, 192, 3, 2, 0, '4 x 4 grid: 32 images per item, ragged'),
    (10, 0, 1493, 17, 17, 16, 192, 3, 2, 0, ''),
    (10, 0, 373, 33, 33, 16, 192, 3, 2, 0, ''),
    (10, 0, 94, 65, 65, 16, 192, 3, 2, 0, '32 x 32 grid: two patches per image'),
    # ragged walks with a constant cout block (two cout blocks, an even stride): 384 items on 256 blocks, one or two per block --
    # the launch pattern of the 16 x 16 layer at batch 128 -- and the same images on F(2x2,3x3): 766 items, two or three per block
    (9, 0, 383, 16, 16, 32, 128, 3, 1, 1, '384 items on 256 blocks: one or two per block, same cout block'),
    (7, 0, 383, 16, 16, 16, 128, 3, 1, 1, '766 items: two or three per block, same cout block'),
]

# the five launches of tests/test_wino_gpu.py that run several items per CU but ONE per block: (path, mode, N, H, W, C, K, k, s, p)
#  -- forward, and the data gradient that test module runs on the same tuple with the channel roles swapped
SINGLE_ITEM_CASES = [
    (7, 0, 40, 16, 16, 16, 64, 3, 1, 1), (7, 1, 40, 16, 16, 64, 16, 3, 1, 1),          # CASES (40, 16, 16, 16, 64)
    (8, 0, 70, 8, 8, 16, 192, 4, 2, 1), (8, 1, 70, 8, 8, 192, 16, 4, 2, 1),            # S2CASES (70, 8, 8, 16, 192)
    (9, 0, 40, 16, 16, 32, 64, 3, 1, 1), (9, 1, 40, 16, 16, 64, 32, 3, 1, 1),          # CASES44 (40, 16, 16, 32, 64)
    (11, 0, 40, 16, 16, 32, 32, 3, 1, 1), (11, 1, 40, 16, 16, 32, 32, 3, 1, 1),        # CASES44N (40, 16, 16, 32, 32)
    (10, 0, 70, 17, 17, 48, 64, 3, 2, 0),                                              # S3CASES (70, 8, 48, 64)
]

# fewest chunks (8 input channels, for one phase) an item of the family can have: the channel rule of the family's ok()
MIN_CHUNKS = {(7, 0): 2, (7, 1): 2, (9, 0): 4, (9, 1): 4, (11, 0): 4, (11, 1): 4, (8, 0): 4, (8, 1): 2, (10, 0): 8}

Geometry = collections.namedtuple('Geometry', 'NP NIMG ppi NSUB chunks groups')


def cdiv(a, b):
    return -(-a // b)


def case_id(case):
    P, m, N, H, W, C, K, k, s, p = case[:10]
    return 'p%d-m%d-%dx%dx%dx%d-%d-k%ds%dp%d' % (P, m, N, H, W, C, K, k, s, p)


def lds(case):
    """(ldx, ldy, ldw): channels + 4."""
    return case[5] + 4, case[6] + 4, case[6] + 4


def round_ok(items, min_items=230):
    """fills_chip(items, min_items, 14, 10): a single partial round from min_items, else a last round not mostly empty."""
    if items < CUS:
        return items >= min_items
    return cdiv(items, CUS) * CUS * 10 <= items * 14


def n32(cout, W, patches):
    """Wino44::n32: 32-wide items when the cout count is not whole 64-wide blocks, on 4x4 maps, and when the 64-wide items do
    not fill the chip while twice as many half items do."""
    if cout % 64 or W == 4:
        return True
    items64 = patches * (cout // 64)
    return not round_ok(items64) and round_ok(2 * items64)


def geometry(case, N=None):
    """Tile blocks, images per tile block, tile blocks per image group, items per tile block, chunks per item, image groups
    of a case (``N``: of a launch of the same layer on N images)."""
    P, mode, N0, H, W, C, K, k, s, p = case[:10]
    N = N0 if N is None else N
    cin, cout = (C, K) if mode == 0 else (K, C)
    if P == 7:                                   # Wino::args
        TH, TW = min(8, H // 2), min(8, W // 2)
        nimg, ppi = 64 // (TH * TW), (H // (2 * TH)) * (W // (2 * TW))
        nsub, chunks = cout // 64, cin // 8
    elif P in (9, 11):                           # Wino44::args
        TW, TH = min(8, W // 4), min(4, H // 4)
        nimg, ppi = 32 // (TH * TW), (H // (4 * TH)) * (W // (4 * TW))
        wide = n32(cout, W, cdiv(N, nimg) * ppi)
        nsub, chunks = (cout // 32 if wide else cout // 64), cin // 8
    elif P == 8:                                 # Wino22::args: whole images, Ho x Wo grid of 2x2 tiles
        Ho, Wo = H // 2, W // 2
        nimg, ppi = 128 // ((Ho // 2) * (Wo // 2)), 1
        nsub = cout // 64 * (4 if mode == 1 else 1)
        chunks = cin // 8 * (1 if mode == 1 else 4)
    elif P == 10:                                # Wino23::args
        Ho, Wo = (H - 1) // 2, (W - 1) // 2
        TW, TH = (16, 8) if Wo >= 32 else (Wo // 2, Ho // 2)
        nimg, ppi = 128 // (TH * TW), (Ho // (2 * TH)) * (Wo // (2 * TW))
        nsub, chunks = cout // 64, 4 * (cin // 8)
    else:
        raise ValueError(P)
    groups = cdiv(N, nimg)
    return Geometry(groups * ppi, nimg, ppi, nsub, chunks, groups)


def family(case, N=None):
    """The path a forced launch of the case's family runs on N images: 9 or 11 by Wino44::n32, else the case's own."""
    P, mode, N0, H, W, C, K = case[:7]
    if P not in (9, 11):
        return P
    g = geometry(case, N)
    return 11 if n32(K if mode == 0 else C, W, g.NP) else 9


def grid(NP, NSUB):
    """persistent_grid(F::items(a, 8))."""
    return 8 * min(CUS // 8, cdiv(NP, 8) * NSUB)


def walk(NP, NSUB, grid_blocks):
    """[(xcd, slot, [(tile block, sub-item), ...])] for every block of the grid, in the order the block runs them."""
    nslots = grid_blocks >> 3
    blocks = []
    for b in range(grid_blocks):
        xcd, slot = b & 7, b >> 3
        L = cdiv(NP - xcd, 8) * NSUB if NP > xcd else 0
        blocks.append((xcd, slot, [((w // NSUB) * 8 + xcd, w % NSUB) for w in range(slot, L, nslots)]))
    return blocks


def xcd_lists(NP, NSUB):
    return [cdiv(NP - x, 8) * NSUB if NP > x else 0 for x in range(8)]


def sub_item(case, sub):
    """(cout block, dx phase) of sub-item ``sub`` (wino22.h decode: the strided data gradient has the phase in the low bits)."""
    if case[0] == 8 and case[1] == 1:
        return sub >> 2, sub & 3
    return sub, 0


def group_permutation(case):
    """Image order with the whole image groups reversed and the ragged group (if any) kept last."""
    g = geometry(case)
    N, full = case[2], case[2] // g.NIMG
    order = []
    for grp in reversed(range(full)):
        order += range(grp * g.NIMG, (grp + 1) * g.NIMG)
    return order + list(range(full * g.NIMG, N))


def sub_launches(case):
    """[(first image, last image + 1)]: the case's images in launches of whole image groups, each so small that its fullest
    XCD list has at most 32 items (every block walks ONE item) and that F(4x4,3x3) chooses the item width of the whole launch
    (family(case, n) == path).  As few launches as that allows: full-sized ones and a remainder, or, where the remainder
    would change the item width, equal pieces below the width rule's window."""
    P, N = case[0], case[2]
    g = geometry(case)
    gmax = (8 * (32 // g.NSUB)) // g.ppi              # image groups whose tile blocks give ceil(NP / 8) * NSUB <= 32
    def keeps_width(n):
        if P != 9:
            return family(case, n) == P
        items64 = geometry(case, n).NP * g.NSUB       # (>= 230 or < 115: outside the window of the rule's third clause)
        return family(case, n) == P and (items64 >= 230 or items64 < 115)

    for per in range(gmax, 0, -1):
        cuts = [(a * g.NIMG, min(N, (a + per) * g.NIMG)) for a in range(0, g.groups, per)]
        if all(keeps_width(b - a) for a, b in cuts):
            return cuts
    raise ValueError('no sub-launch size keeps %s on path %d' % (case_id(case), P))
