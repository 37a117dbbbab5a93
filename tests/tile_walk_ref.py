"""The persistent tile walk of the fused GEMMs (votenet_amd/csrc/mlp_fast.hip), restated in plain Python, and the table of cases
tests/test_gpu_tile_walk.py runs.  No torch, no numpy: tests/test_tile_walk_cpu.py checks the table without a GPU.

plan()      which wave layout fast_dispatch / mlp_linear_pool_launch pick for a shape and how many workgroups (gridDim.x) they launch
schedule()  the row tiles every workgroup of such a launch takes (the top of mlp_linear_fast_kernel)
CASES       (family, rows, cin, cout, gx, chunked, device tile count) + what the family's test needs to build the launch"""
import collections

FG_BM = 128                          # rows of a tile
DEFAULT_CAPS = (512, 1024)           # g_fast_cap22, g_fast_cap41


def plan(rows, cin, cout, epi_pooled=False, narrow_below=False, src_pooled_k=0, xcd_chunk=False, cap22=DEFAULT_CAPS[0],
         cap41=DEFAULT_CAPS[1]):
    """-> (variant, gx, ny): variant "2x2" (128 x 128 tiles, capped at cap22 / ny), "4x1" (128 x 64 tiles, capped at cap41 / ny), "few"
    (128 x 64 tiles, one workgroup per row tile whatever the caps) or "not served" (the entry point raises).
    epi_pooled: the pooled forward layers (EPI 2 / 8: mlp_linear_pool_launch); narrow_below: the input-gradient GEMMs over a narrow
    first layer (EPI 4 / 7); src_pooled_k: the pool width of a pooled upstream gradient (SRC 2), 0 otherwise."""
    if rows <= 0 or rows % FG_BM or cin % 32 or cin > 512:
        return "not served", 0, 0
    ntiles = rows // FG_BM
    if epi_pooled:
        if cout % 128:
            return "not served", 0, 0
        ny = cout // 128
        return "2x2", min(ntiles, cap22 // ny), ny
    if narrow_below:
        if cout % 64:
            return "not served", 0, 0
        ny = cout // 64
        return "4x1", min(ntiles, cap41 // ny), ny
    if cout % 128 == 0 and ntiles * (cout // 128) < 200:
        variant, ny, gx = "few", cout // 64, ntiles
    elif cout % 128 == 0:
        variant, ny = "2x2", cout // 128
        gx = min(ntiles, cap22 // ny)
        if xcd_chunk and gx >= 64:
            gx &= ~7
    elif cout % 64 == 0:
        variant, ny = "4x1", cout // 64
        gx = min(ntiles, cap41 // ny)
    else:
        return "not served", 0, 0
    if src_pooled_k and (gx * FG_BM) % src_pooled_k:
        return "not served", gx, ny  # a tile jump must be a whole number of groups
    return variant, gx, ny


def schedule(ntiles, gx, chunked):
    """-> for every workgroup 0 .. gx-1 the list of row tiles it takes, in the order it takes them.  chunked: the launch asks for
    per-XCD chunks (FastArgs::xcd_chunk); the kernel then chunks whenever gridDim.x is a multiple of 8, also below 64 workgroups."""
    out = []
    for b in range(gx):
        if chunked and gx % 8 == 0:
            per = (ntiles + 7) // 8
            lo = (b & 7) * per
            hi = min(lo + per, ntiles)
            tstride, tile0 = gx >> 3, lo + (b >> 3)
            n = (hi - 1 - tile0) // tstride + 1 if tile0 < hi else 0
        else:
            tstride, tile0 = gx, b
            n = (ntiles - 1 - b) // gx + 1 if b < ntiles else 0
        out.append([tile0 + t * tstride for t in range(n)])
    return out


def walk_lengths(ntiles, gx, chunked):
    return sorted(set(len(w) for w in schedule(ntiles, gx, chunked)))


# family -> how plan() is asked about it, and whether its launches can leave a workgroup without a tile (per-XCD chunks: the piece-layout
# GEMMs that gather the per-point table; a tile count read on the device: the *_half entries that take nh_dev)
Family = collections.namedtuple("Family", "epi_pooled narrow_below can_be_empty what")
FAMILIES = {
    "dense":          Family(False, False, False, "linear_dense with and without statistics (SRC 0, EPI 0 / 1)"),
    "pool":           Family(True, False, False, "linear_dense_pool(k=64) (EPI 2)"),
    "pool_half":      Family(True, False, True, "linear_dense_pool(half=, gamma=) (EPI 8), count on the host and on the device"),
    "linear_half":    Family(False, False, True, "votenet_mlp_linear_half (SRC 0, EPI 1, nh_dev)"),
    "dgrad_half":     Family(False, False, True, "dgrad_bn_half (SRC 5, EPI 1, nh_dev)"),
    "dgrad":          Family(False, False, False, "dgrad_bn(da=) (SRC 1)"),
    "dgrad_pooled":   Family(False, False, False, "dgrad_bn(gout=, argmax=, k=) (SRC 2)"),
    "dgrad_reduce":   Family(False, False, False, "dgrad_bn(below=, below_tail=) (EPI 3)"),
    "narrow":         Family(False, False, False, "narrow_linear(want_mask) (SRC 3): the forward GEMM of the narrow stage tests"),
    "narrow_dgrad":   Family(False, True, False, "narrow_dgrad_bn_reduce, plain and masked (EPI 4 / 7)"),
    "assembled":      Family(False, False, False, "assembled_linear / assembled_dgrad_bn_reduce (SRC 4 / EPI 6)"),
    "assembled_half": Family(False, False, True, "the same with half= (SRC 4 / SRC 5 + EPI 6, xcd_chunk) and dgrad_bn_half"),
}

# rows, cin, cout: of the GEMM; gx: the workgroups along x the walked launch must have (the GPU test sets the cap that gives it and
# plan() confirms it); chunked: votenet_debug_fast_xcd_chunk for the launch (a family that never sets FastArgs::xcd_chunk: False);
# dev_tiles: the tile count the kernel reads on the device (None: rows is exact); k: pool width of SRC 2; geom: key of GEOMETRY; cap: the
# cap to set where it is not gx * ny (the launcher rounds a chunked 2x2 grid of 64 or more down to a multiple of 8)
Case = collections.namedtuple("Case", "family rows cin cout gx chunked dev_tiles k geom cap")

# the geometry-driven families (arguments of the stage helpers in test_gpu_narrow / test_gpu_assembled / test_gpu_half); `tiles` of a piece
# layout follows from the ball query and is asserted on the device (CPU oracle: farthest_point_sample + query_ball_point + half_groups)
GEOMETRY = {
    "narrow":  dict(args=(2, 500, 64, 64, 3, 64, 64), tiles=64),                 # b, n, m, k, c, c0, c1
    "narrow_h": dict(args=(2, 700, 64, 3, 0.5, 0.0), tiles=37),                  # b, n, m, c, radius, b0_shift (c0 = c1 = 64)
    "asm":     dict(args=(1, 400, 32, 64, 16, 64, 64, 0.3), tiles=16),           # b, n, m, k, cf, c0, c1, radius
    "asm_h17": dict(args=(2, 400, 32, 64, 128, 0.62), widths=(64, 64), tiles=17),  # b, n, m, cf, c2, radius; c0, c1
    "asm_h41": dict(args=(2, 600, 64, 128, 128, 0.56), widths=(64, 64), tiles=41),
    "asm_h9":  dict(args=(2, 400, 32, 64, 128, 0.36), widths=(64, 64), tiles=9),
    "asm_h208": dict(args=(2, 2000, 256, 32, 256, 0.4), widths=(128, 128), tiles=208),  # 2x2 tiles: 208 x 128 columns
}


def _c(family, tiles, cin, cout, gx, chunked=False, dev_tiles=None, k=0, geom=None, cap=None):
    return Case(family, tiles * FG_BM, cin, cout, gx, chunked, dev_tiles, k, geom, cap)


def _cases():
    out = []
    # dense forward: the 2x2 layout needs ntiles * cout / 128 >= 200 (101 x 256); the 4x1 layout a cout that is no multiple of 128
    for gx in (101, 1, 2, 3, 5, 100):
        out.append(_c("dense", 101, 32, 256, gx))
    out.append(_c("dense", 101, 512, 256, 3))
    for cin, cout in ((64, 64), (128, 320)):
        for gx in (17, 1, 2, 3, 5, 16):
            out.append(_c("dense", 17, cin, cout, gx))
    for tiles in (1, 2, 3):
        out.append(_c("dense", tiles, 64, 64, 1))
    # pooled forward (64-row groups): tiles {1, 2, 3, 7, 17}
    for cout, cin in ((128, 64), (256, 32)):
        for tiles, gx in ((1, 1), (2, 1), (3, 1), (7, 7), (7, 2), (17, 17), (17, 5), (17, 16)):
            out.append(_c("pool", tiles, cin, cout, gx))
    # pooled forward on the piece layout: count on the host (rows exact) and on the device (rows = 64 G, the kernel stops at the count)
    for cout, cin in ((128, 64), (256, 32)):
        for tiles, gx in ((1, 1), (2, 1), (3, 1), (7, 2), (17, 17), (17, 5), (17, 16)):
            out.append(_c("pool_half", tiles, cin, cout, gx))
        for gx in (16, 5, 3):  # 32 centres: 16 tiles at most, 7 on the device
            out.append(_c("pool_half", 16, cin, cout, gx, dev_tiles=7))
    # the GEMMs that stop at a device count: 64 tiles at most, {0 pieces, 1, 3, 63 tiles} there; default caps and 8 workgroups
    for fam, cin in (("linear_half", 64), ("dgrad_half", 32)):
        for dev_tiles in (0, 1, 3, 63):
            for gx in (64, 8):
                out.append(_c(fam, 64, cin, 64, gx, dev_tiles=dev_tiles))
    # BatchNorm-backward input gradient from a dense upstream gradient
    for gx in (101, 1, 2, 3, 5, 100):
        out.append(_c("dgrad", 101, 32, 256, gx))
    for gx in (17, 1, 2, 3, 5, 16):
        out.append(_c("dgrad", 17, 128, 64, gx))
    # ... from a pooled one: with 3 workgroups a tile jump is 384 rows = 24 / 12 / 6 groups
    for k, cin in ((16, 32), (32, 64), (64, 128)):
        for gx in (17, 3, 2, 16):
            out.append(_c("dgrad_pooled", 17, cin, 64, gx, k=k))
    out.append(_c("dgrad_pooled", 101, 32, 256, 3, k=64))
    out.append(_c("dgrad_pooled", 101, 32, 256, 100, k=64))
    out.append(_c("dgrad_pooled", 9, 32, 64, 9, k=48))   # 1152 rows = 24 groups of 48: served with one tile per workgroup ...
    out.append(_c("dgrad_pooled", 9, 32, 64, 2, k=48))   # ... not with a jump of 256 rows
    # ... with the BatchNorm-backward reduce of the layer below and its coefficient tail
    for gx in (17, 1, 3, 5, 16):
        out.append(_c("dgrad_reduce", 17, 64, 64, gx))
    for gx in (101, 3, 100):
        out.append(_c("dgrad_reduce", 101, 32, 256, gx))
    # the stage helpers: tile counts follow from the geometry
    for gx in (64, 3, 8, 16, 63):
        out.append(_c("narrow", GEOMETRY["narrow"]["tiles"], 64, 64, gx, geom="narrow"))
        out.append(_c("narrow_dgrad", GEOMETRY["narrow"]["tiles"], 64, 64, gx, geom="narrow"))
    for gx in (37, 3, 8, 16, 36):
        out.append(_c("narrow", GEOMETRY["narrow_h"]["tiles"], 64, 64, gx, geom="narrow_h"))
        out.append(_c("narrow_dgrad", GEOMETRY["narrow_h"]["tiles"], 64, 64, gx, geom="narrow_h"))
    for gx in (16, 3, 8, 15):
        out.append(_c("assembled", GEOMETRY["asm"]["tiles"], 64, 64, gx, geom="asm"))
    for geom in ("asm_h17", "asm_h41", "asm_h9"):
        tiles = GEOMETRY[geom]["tiles"]
        out.append(_c("assembled_half", tiles, 64, 64, tiles, chunked=True, geom=geom))
        for gx, chunked in ((8, True), (8, False), (16, True), (16, False), (3, True)):
            if gx < tiles:
                out.append(_c("assembled_half", tiles, 64, 64, gx, chunked=chunked, geom=geom))
    # the 2x2 layout chunked: 208 tiles at one tile per workgroup (208 % 8 == 0: chunks even there), a cap of 70 rounded down to 64
    # workgroups (chunks of 26 tiles, walks of 3 and 4), and the same cap unchunked (70 workgroups, walks of 2 and 3)
    out.append(_c("assembled_half", 208, 128, 128, 208, chunked=True, geom="asm_h208"))
    out.append(_c("assembled_half", 208, 128, 128, 64, chunked=True, geom="asm_h208", cap=70))
    out.append(_c("assembled_half", 208, 128, 128, 70, chunked=False, geom="asm_h208", cap=70))
    return out


CASES = _cases()


def ntiles_of(case):
    """The tiles the kernel walks: the device's count where there is one."""
    return case.rows // FG_BM if case.dev_tiles is None else case.dev_tiles


def plan_of(case, cap22=DEFAULT_CAPS[0], cap41=DEFAULT_CAPS[1]):
    f = FAMILIES[case.family]
    return plan(case.rows, case.cin, case.cout, f.epi_pooled, f.narrow_below, case.k, case.chunked, cap22, cap41)


def caps_of(case):
    """The (cap22, cap41) under which the case's launch has case.gx workgroups along x; the default caps where they already give it."""
    variant, gx, ny = plan_of(case)
    if case.cap is not None:
        return (case.cap, DEFAULT_CAPS[1]) if variant == "2x2" else (DEFAULT_CAPS[0], case.cap)
    if gx == case.gx:
        return DEFAULT_CAPS
    if variant == "2x2":
        return case.gx * ny, DEFAULT_CAPS[1]
    if variant == "4x1":
        return DEFAULT_CAPS[0], case.gx * ny
    raise ValueError("%r: the launch cannot be capped (%s)" % (case, variant))


def is_chunked(case):
    return case.chunked and case.gx % 8 == 0
