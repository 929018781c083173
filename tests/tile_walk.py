"""How the matrix kernels of the two nets hand tiles to their persistent workgroups, restated in Python, and the cases of
test_tile_walk_host.py and test_gpu_tile_walk.py that are built on it.  A plain module: no fixtures, no pytest settings.

Every kernel family sizes its grid from min(tiles, compute units) and lets a workgroup walk a list of tiles, so a workgroup
reaches its second tile -- the halo fetched one tile ahead, the next tile's block-floating-point word, the hand-over between
the wave groups of the pipelined ConvBlock -- only in a launch of more tiles than the chip has CUs:

    family      kernel (csrc)                       tile      grid                  walk
    split-f16   conv3x3h.hip launch_g               16 x 16   min(ntiles, CUs)      grid % 8 == 0: XCD by XCD, t = ntiles*xcd>>3 + (wg>>3),
                                                                                    step grid>>3, up to ntiles*(xcd+1)>>3; else plain stride
    direct      conv3x3.hip launch_v                 8 x 16   min(ntiles, CUs)      plain stride: wg, wg + grid, ...
    winograd    wino3x3.hip launch_w                 8 x 32   min(ntiles, CUs)      plain stride
    convblock   convnext.hip launch_block_t, _pipe  16 x 16   min(ntiles, CUs) up   bands of ceil(ntiles/8) tiles per XCD, t = xcd*band + (wg>>3),
                                                              to a multiple of 8    step grid>>3; a first tile past the band: return at once

with xcd = wg & 7.  The tile list is sequence-major, then tile row, then tile column; the four levels of a handle halve H and W
with floor, as rvdd_create does.  A change of a walk, a tile size or a grid rule changes this restatement in the same commit:
test_tile_walk_host.py holds it to "every tile exactly once" for 1 .. 1300 tiles and shows with three mutants that this check
bites, and it asserts what the GPU cases below are there for, so that such a change cannot hollow them out silently."""
import functools

import torch

import rvdd_oracle as O
import random_weights as RW

TILE = {"split-f16": (16, 16), "direct": (8, 16), "winograd": (8, 32), "convblock": (16, 16)}      # (rows, columns)
FAMILIES = tuple(TILE)
LEVELS = 4
MUTANTS = ("band_end_off_by_one", "xcd_stride_is_grid", "no_early_return")


def level_sizes(H, W):
    return [(H >> l, W >> l) for l in range(LEVELS)]


def tile_grid(family, H, W):
    """-> (tile rows, tile columns) of one H x W map"""
    th, tw = TILE[family]
    return (H + th - 1) // th, (W + tw - 1) // tw


def level_tiles(family, B, H, W):
    """-> the tile count of a launch over the whole batch, per level"""
    return [B * ty * tx for ty, tx in (tile_grid(family, h, w) for h, w in level_sizes(H, W))]


def grid_size(family, ntiles, cus):
    g = min(ntiles, cus)
    return (g + 7) // 8 * 8 if family == "convblock" else g


def cout_split_applies(ntiles, cus):
    """conv3x3h.hip: the 48 -> 48 layers of the split-f16 family run one third of the output channels per workgroup (MT = 1,
    three workgroups per tile, one tile each) where that still leaves a CU per workgroup"""
    return 3 * ntiles <= cus


def walk(family, ntiles, cus, mutant=None):
    """-> per workgroup, the tiles it visits, in order.  mutant: one of MUTANTS, the restatement with that one mistake."""
    assert mutant is None or mutant in MUTANTS, mutant
    grid = grid_size(family, ntiles, cus)
    out = []
    for wg in range(grid):
        xcd = wg & 7
        if family == "convblock":
            per_xcd = (ntiles + 7) >> 3
            band_end = min((xcd + 1) * per_xcd, ntiles) + (mutant == "band_end_off_by_one")
            stride = grid >> 3
            t = xcd * per_xcd + (wg >> 3)
            mine = []
            if t < band_end or mutant == "no_early_return":
                while True:                            # the kernels' loop tests the NEXT tile at the end of the body
                    mine.append(t)
                    t += stride
                    if t >= band_end:
                        break
            out.append(mine)
            continue
        if family == "split-f16" and grid % 8 == 0:
            t, t_end = (ntiles * xcd >> 3) + (wg >> 3), ntiles * (xcd + 1) >> 3
            t_step = grid if mutant == "xcd_stride_is_grid" else grid >> 3
        else:
            t, t_end, t_step = wg, ntiles, grid
        out.append(list(range(t, t_end, t_step)))
    return out


def visits_each_tile_once(walks, ntiles):
    return sorted(t for w in walks for t in w) == list(range(ntiles))


def locate(tile, ty, tx):
    """tile index of a launch whose maps have ty x tx tiles -> (sequence, tile row, tile column)"""
    b, rr = divmod(tile, ty * tx)
    return (b,) + divmod(rr, tx)


def is_interior(family, tile, H, W):
    """the tile touches no border of its H x W image: full, and with a neighbour on every side"""
    th, tw = TILE[family]
    ty, tx = tile_grid(family, H, W)
    _, r, c = locate(tile, ty, tx)
    return 0 < r and (r + 2) * th <= H and 0 < c and (c + 2) * tw <= W


def visitor(family, ntiles, cus, tile):
    """-> (workgroup, the position of `tile` in its walk from 0, the length of that walk)"""
    for wg, w in enumerate(walk(family, ntiles, cus)):
        if tile in w:
            return wg, w.index(tile), len(w)
    raise ValueError((family, ntiles, cus, tile))


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# A: the smallest frames whose four levels all have a tile of every family, in the smallest batch that puts every level of every
#    family past the CU count, with a remainder mod 8: B = CUs + 3 of 18 x 34 (levels 9 x 17, 4 x 8, 2 x 4: every decoder stage
#    zero-pads).  B: 80 x 112 frames, 35 split-f16 tiles each, interior tiles and row changes inside one workgroup's walk; the
#    largest batch that leaves levels 1 .. 3 of every family (20 direct tiles per frame at level 1) with one tile per workgroup:
#    12 at 256 CUs.
def case_a(cus):
    return cus + 3, 18, 34


def case_b(cus):
    return cus // 20, 80, 112


CASES = {"A": case_a, "B": case_b}


def chunk_batch(case, family, cus):
    """The batch of the reference handles: the largest in which no launch of `family` (nor of the split-f16 kernels that a
    handle of another family still runs) has more tiles than CUs -- every workgroup one tile, the regime that
    test_gpu_random_weights.py holds to f64.  Case A: (CUs - 1) // tiles per frame, 42 at 256 CUs (28 for the direct kernel with its nine
    8 x 16 tiles per 18 x 34 frame); case B: two halves (four quarters for the direct kernel)."""
    B, H, W = CASES[case](cus)
    per_frame = max(level_tiles(f, 1, H, W)[0] for f in (family, "split-f16"))
    n = (cus - 1) // per_frame
    assert n >= 1, ("a single frame has more tiles than the device has CUs", case, family, cus)
    if case == "B":
        while B % n:
            n -= 1
    return n


def chunks(case, family, cus):
    """-> [(first sequence, count)] of the reference runs: whole chunks, then the remainder"""
    B = CASES[case](cus)[0]
    n = chunk_batch(case, family, cus)
    return [(b, min(n, B - b)) for b in range(0, B, n)]


def premises(case, cus):
    """What the case is there for, from the rules above -> (rows of the table, list of the premises that do not hold).
    One row per family and level: tiles, grid, workgroups without a tile, fewest and most tiles of the others."""
    B, H, W = CASES[case](cus)
    rows, bad = [], []
    need = lambda ok, *what: None if ok else bad.append((case, cus) + what)
    for fam in FAMILIES:
        nt = level_tiles(fam, B, H, W)
        for lvl, n in enumerate(nt):
            w = walk(fam, n, cus)
            need(visits_each_tile_once(w, n), fam, lvl, "walk")
            lens = [len(x) for x in w]
            busy = [k for k in lens if k]
            rows.append((case, fam, lvl, n, len(w), lens.count(0), min(busy), max(busy),
                         cout_split_applies(n, cus) if fam == "split-f16" else None))
            if case == "A":
                need(n > cus, fam, lvl, "more tiles than CUs")
            elif lvl == 0:
                need(n > cus, fam, lvl, "more tiles than CUs")
            else:
                need(n <= cus, fam, lvl, "one tile per workgroup below level 0")
        if case == "A":
            need(any(n % 8 for n in nt), fam, "a level with ntiles % 8 != 0")
            last = [len(x) for x in walk(fam, nt[-1], cus)]
            need(1 in last and 2 in last, fam, "coarsest level: workgroups with one tile and with two")
            need(max(len(x) for x in walk(fam, nt[0], cus)) >= 5, fam, "level 0: a workgroup with 5 tiles")
            if fam == "convblock":
                need(any(0 in [len(x) for x in walk(fam, n, cus)] for n in nt), fam, "a workgroup without a tile")
        else:
            hit = False
            for w in walk(fam, nt[0], cus):
                for t, u in zip(w, w[1:]):
                    per = nt[0] // B
                    hit |= t // per != u // per and is_interior(fam, t, H, W) and is_interior(fam, u, H, W)
            need(hit, fam, "consecutive interior tiles of two sequences in one walk")
        # the reference runs: one tile per workgroup at every level, in every family the handle may launch
        for n in set(c for _, c in chunks(case, fam, cus)):
            for f2 in (fam, "split-f16"):
                need(max(level_tiles(f2, n, H, W)) <= cus, fam, f2, n, "reference handle: at most one tile per workgroup")
    if case == "A":                                      # between them the reference handles take the output-channel split both ways
        sizes = set(c for _, c in chunks("A", "split-f16", cus))
        took = set(cout_split_applies(n, cus) for c in sizes for n in level_tiles("split-f16", c, H, W))
        need(took == {True, False}, "split-f16", "reference handles with and without the output-channel split")
    return rows, bad


def premises_table(rows):
    head = "case family      level  tiles  grid  idle  tiles/workgroup  cout split"
    return "\n".join([head] + [f"{c:<4} {f:<11} {l:>5} {n:>6} {g:>5} {z:>5}  {lo:>6} .. {hi:<6} {'' if s is None else 'yes' if s else 'no'}"
                              for c, f, l, n, g, z, lo, hi, s in rows])


# ---- the forward cases and the reference they share --------------------------------------------------------------------------------
# (arch, checkpoint stem, future frame): the nets of test_gpu_random_weights.py
UNETS = (("convunet", "recurrent-convunet-iso3200", 0), ("convunet", "recurrent-convunet-future-iso3200", 1),
         ("convunet+feat", "recurrent-convunet+feat-iso3200", 0), ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1))
NEXTS = (("next", "recurrent-ConvNeXtUnet-iso3200", 0), ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1))
UNET_CASES = tuple((p, c) for p in ("he", "pow2") for c in "AB")
NEXT_CASES = (("pow2", "A"), ("he", "B"))      # the f64 oracle of the ConvNeXt nets is the slow one: one profile per case
SEED = 3


@functools.lru_cache(maxsize=2)
def forward_reference(stem, profile, case, cus):
    """-> (weights, x, feat_in, the f64 oracle's (out, feat_out), e_ref of each): computed once per case, shared by every form of
    the net, and never written to"""
    B, H, W = CASES[case](cus)
    sd = RW.random_state_dict(stem, SEED, profile)
    x, f = RW.net_inputs(B, O.net_input_nc(sd), H, W, 1000 * SEED + H, O.net_has_feat(sd))
    with torch.no_grad():
        o32 = O.net_forward(sd, x, f)
        o64 = O.net_forward(RW.to64(sd), x.double(), None if f is None else f.double())
    return sd, x, f, o64, [None if a is None else RW.rel_err(a, b) for a, b in zip(o32, o64)]
