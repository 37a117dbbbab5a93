"""BatchNorm batch statistics: the float64 reference, the metric the GPU tests bound, a CPU model of the fp32 accumulation order of the
GEMM epilogues, and the input builders tests/test_gpu_bn_stats.py and tests/test_bn_stats_cpu.py share.  numpy and torch only; the
package is not imported.

reference()  two-pass float64 mean and biased variance of a (rows, c) z, optionally with row weights (the piece layout)
metric()     e = max |a_dev - a_ref| / max(1, max |a_ref|) for a = gamma (z - mean) / sqrt(var + eps) + beta, a_dev = z scale + shift
             formed in float64 from the recorded fp32 scale / shift: the project's bar shape on what BatchNorm hands on
finalize()   bn_finalize_kernel's arithmetic (csrc/mlp.hip) on a pair of raw sums
emulate()    (sum z, sum z^2) the way the epilogues accumulate them: sequential fp32 lane partials of L elements, an fp32 combine of
             `waves` partials, then double.  A model of an implementation -- nothing calibrates it against the device.
r of a channel: |mean| / std."""
import collections

import numpy as np
import torch

BN_EPS = 1e-5
BAR = 1e-5            # the project's bar on a module's output (tests/test_gpu_model.py)
CONDITION = 2.5e-6    # what the emulation must stay under where the bar is asserted of an input-sourced case: a factor of four
SEEDS = 8
ACT_LIMIT, W_LIMIT = 4094.0, 255.0  # the fp16 x 2 forms' operand range


# --------------------------------------------------------------------------------------------------------------- reference and metric


def reference(z, weights=None):
    """z (rows, c), weights (rows,) or None -> (mean, var, n): float64, two passes, biased variance; a row of weight w counts w times."""
    z = np.asarray(z, np.float64)
    w = np.ones(z.shape[0]) if weights is None else np.asarray(weights, np.float64)
    n = w.sum()
    mean = (z * w[:, None]).sum(0) / n
    d = z - mean
    return mean, (d * d * w[:, None]).sum(0) / n, n


def metric(z, scale, shift, gamma, beta, weights=None, eps=BN_EPS):
    """-> dict: e (c,) per channel, each over the launch's max(1, max |a_ref|); var_rel (c,) relative error of the variance the recorded
    scale implies (gamma != 0), r (c,) of the reference.  z: what the reference is taken from (float64 internally)."""
    z = np.asarray(z, np.float64)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    scale, shift = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    mean, var, _ = reference(z, weights)
    a_ref = gamma * (z - mean) / np.sqrt(var + eps) + beta
    a_dev = z * scale + shift
    den = max(1.0, float(np.abs(a_ref).max()))
    with np.errstate(divide="ignore", invalid="ignore"):
        var_dev = (gamma / scale) ** 2 - eps
        var_rel = np.where(var > 0, np.abs(var_dev - var) / np.where(var > 0, var, 1.0), 0.0)
        r = np.where(var > 0, np.abs(mean) / np.sqrt(np.where(var > 0, var, 1.0)), np.inf)
    return dict(e=np.abs(a_dev - a_ref).max(0) / den, var_rel=var_rel, r=r, mean=mean, var=var)


def recorded_errors(mean_dev, var_dev, z, weights=None):
    """For the record: relative error of the recorded variance and absolute error of mean / std, per channel (var > 0)."""
    mean, var, _ = reference(z, weights)
    ok = var > 0
    sd = np.sqrt(np.where(ok, var, 1.0))
    return (np.where(ok, np.abs(np.asarray(var_dev, np.float64) - var) / np.where(ok, var, 1.0), 0.0),
            np.where(ok, np.abs(np.asarray(mean_dev, np.float64) - mean) / sd, 0.0))


def finalize(s1, s2, n, gamma, beta, eps=BN_EPS):
    """bn_finalize_kernel: the subtraction in double, the clamp, scale in fp32 from the fp32 variance, shift = beta - mean scale in double
    from the double mean, rounded once -> scale, shift, mean, var (float32)."""
    mu = np.asarray(s1, np.float64) / float(n)
    v = np.asarray(s2, np.float64) / float(n) - mu * mu
    v = np.where((v < 0) | (float(n) == 1.0), 0.0, v)
    muf, vf = mu.astype(np.float32), v.astype(np.float32)
    sc = np.asarray(gamma, np.float32) / np.sqrt(vf + np.float32(eps))
    sh = (np.asarray(beta, np.float32).astype(np.float64) - mu * sc.astype(np.float64)).astype(np.float32)  # one rounding
    return sc, sh, muf, vf


# ------------------------------------------------------------------------------------------------------------------------ emulation


def emulate(z, L, waves=4, pivot=False):
    """z (rows, c) -> (sum z, sum z^2) float64 (c,).  Rows are dealt to lanes in runs of L consecutive rows; a lane adds v and v * v to
    two fp32 partials in row order.  pivot=False, the epilogues before the pivot: `waves` consecutive lanes' partials are added in
    fp32, the results in double (the table of DESIGN.md).  pivot=True, the epilogues as they are: a lane adds d = v - c and d * d, c
    its first v cut to eight significant bits, and comes back to double by itself, sum z = s1 + n c, sum z^2 = s2 + 2 c s1 + n c^2;
    `waves` lanes are added in double and their two sums cut to 24 bits -- to 36 where the |mean| of their rows is 8 std or more."""
    z = np.asarray(z, np.float32)
    rows, c = z.shape
    lanes = -(-rows // L)
    lanes = -(-lanes // waves) * waves
    zp = np.zeros((lanes * L, c), np.float32)
    zp[:rows] = z
    zp = zp.reshape(lanes, L, c)
    count = np.clip(rows - np.arange(lanes) * L, 0, L).astype(np.float64)[:, None]
    piv = (zp[:, 0].view(np.uint32) & np.uint32(0xffff0000)).view(np.float32) if pivot else np.zeros((lanes, c), np.float32)
    s1 = np.zeros((lanes, c), np.float32)
    s2 = np.zeros((lanes, c), np.float32)
    for i in range(L):
        live = (i < count).astype(np.float32)  # rows past the end add nothing
        v = (zp[:, i] - piv) * live
        s1 = s1 + v
        s2 = s2 + v * v
    if pivot:  # (stat_unpivot, stat_cut of csrc/mlp_types.h)
        p, d1, d2 = piv.astype(np.float64), s1.astype(np.float64), s2.astype(np.float64)
        group = lambda t: t.reshape(lanes // waves, waves, -1).sum(1)
        t1, t2, n = group(d1 + count * p), group(d2 + 2.0 * p * d1 + count * p * p), group(count)
        long_ = t1 * t1 >= 64.0 * (n * t2 - t1 * t1)

        def cut(t):
            g = t * 131073.0
            return np.where(long_, g - (g - t), t.astype(np.float32).astype(np.float64))
        return cut(t1).sum(0), cut(t2).sum(0)
    w1 = np.zeros((lanes // waves, c), np.float32)
    w2 = np.zeros((lanes // waves, c), np.float32)
    for k in range(waves):
        w1 = w1 + s1.reshape(lanes // waves, waves, c)[:, k]
        w2 = w2 + s2.reshape(lanes // waves, waves, c)[:, k]
    return w1.astype(np.float64).sum(0), w2.astype(np.float64).sum(0)


def emulated_e(z, L, waves=4, gamma=None, beta=None, pivot=False):
    """The metric of the emulated sums of z, finalized as the device finalizes -> e (c,)."""
    z = np.asarray(z, np.float32)
    c = z.shape[1]
    gamma = np.ones(c, np.float32) if gamma is None else gamma
    beta = np.zeros(c, np.float32) if beta is None else beta
    s1, s2 = emulate(z, L, waves, pivot)
    sc, sh, _, _ = finalize(s1, s2, z.shape[0], gamma, beta)
    return metric(z, sc, sh, gamma, beta)["e"]


_table = {}


def table_e(rows, r, L, waves=4):
    """The table of DESIGN.md: max over SEEDS draws of z ~ N(r, 1) (rows,) of the emulated e, fp32 partials WITHOUT a pivot (what the
    issue that set the Tier B bars measured).  Memoised: the Tier B bars read it."""
    key = (rows, float(r), L, waves)
    if key not in _table:
        z = np.stack([np.random.default_rng(1000 + s).normal(r, 1.0, rows) for s in range(SEEDS)], 1)
        _table[key] = float(emulated_e(z, L, waves).max())
    return _table[key]


# ------------------------------------------------------------------------------------------------------------------- input builders
# A launch mixes columns: every column has a target r, a magnitude (std of z) and a kind.  Tier A targets are asserted at the bar, Tier B
# targets at the smaller of the bar and four times the unpivoted emulation's maximum; `const` is a column whose z is one value in every
# row that eight bits hold (1.5, or 0 without a bias: the pivot is z itself and every partial is zero); `constg` one whose value they do
# not hold (1.2345, or a small bias: the partials carry z - c != 0 and its rounded squares).

Column = collections.namedtuple("Column", "r sigma kind")
CONST_VALUE = {"const": 1.5, "constg": 1.2345}
BIAS_COLUMNS = [Column(0, 1, "r"), Column(3, 1, "r"), Column(10, 1, "r"), Column(50, 1, "r"), Column(300, 1, "r"),
                Column(0, 0, "const"), Column(3, 1e-3, "r"), Column(3, 30, "r"), Column(0, 0, "constg")]
INPUT_COLUMNS = [Column(0, 1, "r"), Column(3, 1, "r"), Column(10, 1, "r"), Column(30, 1, "r"), Column(100, 1, "r"),
                 Column(0, 0, "const"), Column(3, 1e-3, "r"), Column(3, 30, "r")]
DOUBLE_INPUT_COLUMNS = INPUT_COLUMNS[:5] + [Column(300, 1, "r")] + INPUT_COLUMNS[5:]  # the double-precision producers: up to 300
LADDER = (2.0, 8.0, 40.0, 200.0, 800.0)  # offsets of the nonnegative activations relu(q + N(0, 1)): |mean| / std of one input is ~q


def levels(cin):
    """The ladder level of every input: k % 5; fewer than five inputs are spread over the whole ladder."""
    if cin >= len(LADDER):
        return np.arange(cin) % len(LADDER)
    return np.round(np.arange(cin) * (len(LADDER) - 1.0) / max(1, cin - 1)).astype(np.int64)


def ladder(cin):
    return torch.tensor([LADDER[lv] for lv in levels(cin)])


def columns_of(source, cout, double=False, zero=True):
    """zero=False: without the input-sourced r = 0 column (too few inputs for a zero-sum column: the narrow layer's five features)."""
    pat = BIAS_COLUMNS if source == "bias" else (DOUBLE_INPUT_COLUMNS if double else INPUT_COLUMNS)
    if source == "input" and not zero:
        pat = pat[1:]
    return [pat[j % len(pat)] for j in range(cout)]


def _r_of(z, weights=None):
    mean, var, _ = reference(z, weights)
    return np.abs(mean) / np.sqrt(var)


def bias_case(rows, cin, cout, seed, act=None, weights=None):
    """source "bias": random activations (rows, cin) -- or `act`, what the GEMM's loader hands on -- and zero-mean weights; then
    b = r sigma_col - mean_col from the float64 product, so that a column's mean is r sigma_col exactly (a BatchNorm is invariant to
    it).  -> x (None when act is given), w, b float32 tensors, the columns."""
    g = torch.Generator().manual_seed(seed)
    x = None
    if act is None:
        x = torch.randn(rows, cin, generator=g)
        act = x
    cols = columns_of("bias", cout)
    w = torch.randn(cin, cout, generator=g) * (2.0 / cin) ** 0.5
    b = torch.zeros(cout)
    a64 = act.double().numpy()
    for j, col in enumerate(cols):
        if col.kind in CONST_VALUE:
            w[:, j] = 0.0
            b[j] = CONST_VALUE[col.kind]
    mean, var, _ = reference(a64 @ w.double().numpy(), weights)
    for j, col in enumerate(cols):
        if col.kind == "r":
            s = col.sigma / np.sqrt(var[j])
            w[:, j] *= s
            b[j] = col.r * col.sigma - mean[j] * s
    return x, w.float().contiguous(), b.float().contiguous(), cols


def ladder_activations(rows, cin, seed):
    """Nonnegative activations the way a trained layer behind a ReLU hands them on: input k is relu(q_k + N(0, 1)), q_k from LADDER
    (level k % 5).  -> x ~ N(0, 1) (rows, cin), in_scale = 1, in_shift = q: the folded form; relu(x + q) is the activation."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cin, generator=g)
    return x, torch.ones(cin), ladder(cin)


def one_sign_columns(act, cols, seed, weights=None):
    """source "input": act (rows, cin) >= 0 float64 -> w (cin, len(cols)) float32, every column of one sign (>= 0; signs alternate
    between columns), scaled and mixed so that the measured r of act @ w[:, j] is the column's target.  The mix: nested sets of inputs
    U_0 = {input 0} < U_1 = level 0 < U_2 = levels 0..1 < ... with uniform weights have growing r; the column is
    (1 - t) u_i + t u_(i+1) between the two sets that bracket the target, t by bisection.  r = 0 cannot come from one sign: that
    column alone has zero-sum weights of both signs."""
    rows, cin = act.shape
    g = torch.Generator().manual_seed(seed)
    level = levels(cin)
    sets = [np.zeros(cin)]
    sets[0][0] = 1.0
    for lv in range(len(LADDER)):
        if (level <= lv).sum() > sets[-1].sum():
            sets.append((level <= lv).astype(np.float64))
    zs = act @ np.stack(sets, 1)
    rs = _r_of(zs, weights)
    w = np.zeros((cin, len(cols)))
    for j, col in enumerate(cols):
        if col.kind in CONST_VALUE:
            continue
        if col.r == 0:
            m0 = reference(act, weights)[0] * (level == 0)  # mixed signs on the inputs of the lowest level, orthogonal to their means
            assert (level == 0).sum() >= 2, "an r = 0 column needs two inputs of the lowest level"
            v = torch.randn(cin, generator=g).double().numpy() * (level == 0)
            v = v - m0 * (v @ m0) / (m0 @ m0)
        else:
            i = int(np.searchsorted(rs, col.r)) - 1
            assert 0 <= i < len(sets) - 1, "target r %g outside what these activations reach (%g .. %g)" % (col.r, rs[0], rs[-1])
            lo, hi = 0.0, 1.0
            for _ in range(50):
                t = 0.5 * (lo + hi)
                if _r_of(((1 - t) * zs[:, i] + t * zs[:, i + 1])[:, None], weights)[0] < col.r:
                    lo = t
                else:
                    hi = t
            v = (1 - lo) * sets[i] + lo * sets[i + 1]
        sd = np.sqrt(reference((act @ v)[:, None], weights)[1][0])
        w[:, j] = v * (col.sigma / sd) * (-1.0 if j % 2 else 1.0)
    return torch.from_numpy(w).float().contiguous()


def input_case(rows, cin, cout, seed, double=False, weights=None):
    """source "input" for a dense layer with the BatchNorm + ReLU below it folded into the load: -> x, in_scale, in_shift, w, cols."""
    x, sc, sh = ladder_activations(rows, cin, seed)
    act = torch.relu(x * sc + sh)  # the loader's fp32 arithmetic
    cols = columns_of("input", cout, double)
    w = one_sign_columns(act.double().numpy(), cols, seed + 1, weights)
    return x, sc, sh, w, cols


def measured_r(z, cols, weights=None):
    """-> (r measured per column, target per column) over the `r` columns."""
    r = _r_of(np.asarray(z, np.float64), weights)
    keep = [j for j, c in enumerate(cols) if c.kind == "r"]
    return r[keep], np.array([cols[j].r for j in keep], np.float64)


# --------------------------------------------------------------------------------------------------------------- the matrix of cases
# What tests/test_gpu_bn_stats.py launches, built on the host so that tests/test_bn_stats_cpu.py can check, without a device, the
# conditions its bars rest on.  producer: the Python entry of votenet_amd/mlp.py; gx: workgroups along x of the walked launch (None: the
# default caps, one tile per workgroup at these sizes); fold: "none" or "pend" (a PendingBN folded into the load); opt: per producer.

Case = __import__("collections").namedtuple("Case", "producer rows cin cout gx fold opt")
PER_TILE = {"2x2": 32, "4x1": 16, "few": 16}  # accumulator elements a lane adds per row tile and column
SOURCES = ("bias", "input")


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, opt=tuple(sorted(k.items()))))
    # the fp32 MFMA kernel of csrc/mlp.hip: shapes the fast path does not serve
    for rows, cin, cout in ((5, 3, 7), (130, 128, 79), (777, 48, 79), (1, 3, 7)):
        add("dense_fp32", rows, cin, cout, None, "none")
    # the fast path, 4x1 (cout 64), "few" (cout 128 below 200 tiles: never capped) and 2x2 (101 tiles x 256 columns)
    for fold in ("none", "pend"):
        add("dense", 128, 32, 64, None, fold)
        add("dense", 256, 64, 64, None, fold)
        add("dense", 4096, 64, 64, 4, fold)       # walks of 8 tiles
        add("dense", 128, 32, 128, None, fold)    # few
        add("dense", 256, 256, 128, None, fold)   # few
        add("dense", 101 * 128, 32, 256, None, fold)
        add("dense", 101 * 128, 32, 256, 13, fold)  # walks of 7 and 8 tiles
    add("dense", 4096, 64, 64, 4, "pend", deterministic=True)
    # the pooled forward: always 2x2
    for keep_z in (True, False):
        add("pool", 128, 32, 128, None, "none", keep_z=keep_z)
        add("pool", 256, 64, 128, None, "pend", keep_z=keep_z)
        add("pool", 4096, 256, 128, 4, "pend", keep_z=keep_z)   # walks of 8 tiles
    add("pool", 4096, 32, 128, 1, "none", keep_z=True)          # one workgroup walks 32 tiles: L = 1024
    # the piece layout: rows = the compact rows the launch is sized for
    add("pieces", 384, 64, 128, None, "pend", kind="mixed")
    add("pieces", 512, 32, 128, None, "none", kind="full")
    add("pieces", 256, 32, 128, None, "none", kind="one")
    add("pieces", 2048, 64, 128, 2, "pend", kind="mixed")       # 16 tiles, walks of 8
    add("pieces", 2048, 64, 128, None, "pend", kind="device")   # count on the device: 7 of 16 tiles
    add("pieces", 2048, 64, 128, 1, "pend", kind="device")      # ... one workgroup walks the 7
    # first layers: rows = b m k of a random grouping; cin = 3 + the feature channels
    add("gather", 640, 16, 64, None, "none", geom=(2, 300, 20, 16))
    add("gather", 35, 8, 79, None, "none", geom=(1, 100, 7, 5))
    add("group_linear", 640, 16, 64, None, "none", geom=(2, 300, 20, 16))
    add("group_linear", 4224, 32, 128, None, "none", geom=(1, 500, 66, 64))
    for gx in (None, 2):
        add("assembled", 2048, 32, 64, gx, "none", geom=(1, 300, 32, 64))
        add("narrow", 2048, 8, 64, gx, "none", geom=(1, 300, 32, 64))
    add("assembled", 128, 32, 64, None, "none", geom=(1, 400, 8, 16))
    add("narrow", 128, 8, 64, None, "none", geom=(1, 400, 8, 16))
    # input-sourced r beside a small random bias (the packed epilogues carry the pivot IN the bias): 4x1, few, 2x2, the piece layout
    add("dense", 128, 32, 64, None, "none", small_bias=True)
    add("dense", 4096, 64, 64, 4, "pend", small_bias=True)
    add("dense", 256, 256, 128, None, "pend", small_bias=True)
    add("dense", 101 * 128, 32, 256, None, "none", small_bias=True)
    add("dense", 101 * 128, 32, 256, 13, "pend", small_bias=True)
    add("pool", 4096, 256, 128, 4, "pend", keep_z=True, small_bias=True)
    add("pieces", 384, 64, 128, None, "pend", kind="mixed", small_bias=True)
    add("pieces", 2048, 64, 128, 2, "pend", kind="mixed", small_bias=True)
    return out


CASES = _cases()
C1 = 64  # width of the second layer that consumes a never-stored first layer
DOUBLE_PRODUCERS = ("assembled", "narrow")   # assemble_stats_kernel, narrow_stats: sums formed in double from moments
FAST_PRODUCERS = ("dense", "pool", "pieces", "assembled", "narrow")


def opt(case, key, default=None):
    return dict(case.opt).get(key, default)


def case_id(case, source, L):
    walk = "one-tile" if case.gx is None else "walked-gx%d" % case.gx
    extra = "".join("-%s" % (v if not isinstance(v, bool) else ("%s%d" % (k, v))) for k, v in case.opt if k != "geom")
    return "%s-%dx%dx%d-%s-%s%s-%s-L%s" % (case.producer, case.rows, case.cin, case.cout, walk, case.fold, extra, source, L)


def tier_of(case, source, col, L):
    """-> "A" (e <= BAR), "B" (e <= the smaller of BAR and 4 x the unpivoted emulation's maximum), "exact" (a constant channel that
    eight bits hold: var == 0) or "near" (one they do not: var within 1e-9 of mean^2)."""
    if col.kind in CONST_VALUE:
        return "exact" if col.kind == "const" else "near"
    if case.producer in DOUBLE_PRODUCERS or source == "bias":
        return "A"
    return "A" if (L <= 256 and col.r <= 10) else "B"


def sources_of(case):
    """A case with a small bias beside input-sourced r has no bias-sourced form."""
    return ("input",) if opt(case, "small_bias") else SOURCES


def piece_layout(kind, rows):
    """-> (pts_cnt (G,) int32, pieces kept, device_count).  A ball of pts_cnt points keeps ceil(pts_cnt / 16) of its 4 pieces."""
    tiles = rows // 128
    if kind == "full":
        return np.full(rows // 64, 64, np.int32), rows // 16, False
    if kind == "one":
        return np.full(rows // 16, 5, np.int32), rows // 16, False
    if kind == "device":
        G, pieces = rows // 64, 7 * 8
    else:
        G, pieces = 8 * ((3 * tiles + 7) // 8), tiles * 8
    extra = pieces - G
    three = extra // 2
    cnt = np.full(G, 5, np.int32)
    cnt[(np.arange(three) * G) // max(1, three)] = 40
    if extra % 2:
        cnt[np.flatnonzero(cnt == 5)[-1]] = 20
    return cnt, pieces, kind == "device"


def piece_weights(cnt):
    """The row weights of the compact layout votenet_half_groups makes of pts_cnt, restated: first pieces in centre order, then the
    further kept pieces in centre order; row 0 of a ball's first piece also stands for the 16 rows of each dropped piece."""
    kept = -(-cnt.astype(np.int64) // 16)
    w = np.ones((int(kept.sum()), 16))
    w[:len(cnt), 0] = 1 + 16 * (4 - kept)
    return w.reshape(-1)


def _fold_vectors(cin, seed, source):
    """The BatchNorm folded into the load -> (scale, shift, gamma0, beta0, stats0 per row): stats0 = (0, n) is mean 0 and variance 1."""
    g = torch.Generator().manual_seed(seed)
    if source == "input":
        sc, sh = torch.ones(cin), ladder(cin)
    else:
        sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
    gamma0 = (sc.double() * (1.0 + BN_EPS) ** 0.5).float()
    return gamma0, sh


def host_inputs(case, source):
    """Everything of a case that does not need the device -> dict.  `act` (rows, cin) float32: what the GEMM multiplies; z64 = the float64
    product (+ bias) of act and w; cols; weights (compact rows) or None; n = the rows BatchNorm counts."""
    seed = 100003 * CASES.index(case) + (0 if source == "bias" else 7)
    g = torch.Generator().manual_seed(seed)
    rows, cin, cout = case.rows, case.cin, case.cout
    d = dict(weights=None, n=rows, valid=rows)
    double = case.producer in DOUBLE_PRODUCERS
    if case.producer == "pieces":
        cnt, pieces, device_count = piece_layout(opt(case, "kind"), rows)
        d.update(cnt=cnt, pieces=pieces, device_count=device_count, valid=16 * pieces, n=64 * len(cnt))
        d["weights"] = piece_weights(cnt)
        assert d["weights"].shape[0] == d["valid"] and d["weights"].sum() == d["n"]
    valid = d["valid"]
    geom = opt(case, "geom")
    if geom is None:
        x = torch.randn(rows, cin, generator=g)
        if source == "input" and case.fold == "none":
            x = torch.relu(x + ladder(cin))  # the activation itself, not folded
        if case.fold == "pend":
            gamma0, beta0 = _fold_vectors(cin, seed + 3, source)
            sc0, sh0, _, _ = finalize(np.zeros(cin), np.full(cin, float(rows)), rows, gamma0.numpy(), beta0.numpy())
            act = torch.relu(x * torch.from_numpy(sc0) + torch.from_numpy(sh0))
            d.update(gamma0=gamma0, beta0=beta0)
        else:
            act = x
        d.update(x=x)
    else:
        b, n, m, k = geom
        assert b * m * k == rows
        c = cin - 3
        xyz = torch.rand(b, n, 3, generator=g)
        new_xyz = torch.rand(b, m, 3, generator=g)
        idx = torch.randint(0, n, (b, m, k), generator=g, dtype=torch.int32)
        feat = torch.randn(b, n, c, generator=g)
        if source == "input":
            feat = torch.relu(feat + ladder(c))
        bi = torch.arange(b)[:, None, None]
        dx = (xyz[bi, idx.long()] - new_xyz[:, :, None, :]).reshape(rows, 3)
        act = torch.cat([dx, feat[bi, idx.long()].reshape(rows, c)], 1)
        d.update(xyz=xyz, new_xyz=new_xyz, idx=idx, feat=feat, prow=(idx.long() + torch.arange(b)[:, None, None] * n).reshape(rows))
    a64 = act.double().numpy()[:valid]
    if valid == 1:  # one row: every channel is constant
        cols = [Column(0, 0, "const")] * cout
        w, bias = torch.randn(cin, cout, generator=g), torch.randn(cout, generator=g)
    elif source == "bias":
        _, w, bias, cols = bias_case(valid, cin, cout, seed + 1, act=act[:valid], weights=d["weights"])
    else:
        cols = columns_of("input", cout, double, zero=(levels(cin if geom is None else cin - 3) == 0).sum() >= 2)
        bias = None
        if opt(case, "small_bias"):  # an ordinary small bias beside the inputs' r: at most 0.05 std of the column, either sign
            bias = (torch.rand(cout, generator=g) * 2 - 1) * 0.05 * torch.tensor([col.sigma if col.sigma > 0 else 0.25 for col in cols])
            cols = [col._replace(kind="constg") if col.kind == "const" else col for col in cols]
        if geom is None:
            w = one_sign_columns(a64, cols, seed + 1, d["weights"])
        else:  # the features carry r; the three offset rows (signed by nature) get small weights of both signs
            wf = one_sign_columns(a64[:, 3:], cols, seed + 1)
            sig = torch.tensor([col.sigma for col in cols])
            w = torch.cat([torch.randn(3, cout, generator=g) * 0.05 * sig, wf], 0).float().contiguous()
    if bias is not None:
        bias = bias.float().contiguous()
    z64 = a64 @ w.double().numpy() + (0.0 if bias is None else bias.double().numpy())
    d.update(act=act, w=w, bias=bias, cols=cols, z64=z64)
    gg = torch.Generator().manual_seed(seed + 2)
    d["gamma"] = torch.randn(cout, generator=gg) * 0.3 + 1.0
    d["beta"] = torch.randn(cout, generator=gg) * 0.2
    return d


def lane_run(case):
    """-> (L, variant, caps): the longest run of accumulator elements a lane adds in fp32 before the flush, per column, the wave layout
    and the (cap22, cap41) that give the case's gx.  Fast path: PER_TILE x the longest walk (tests/tile_walk_ref.py: plan, schedule).
    csrc/mlp.hip (dense_fp32, gather; at most 1024 workgroups, one tile each at these sizes): 32 (2x2, cout > 64) or 16; group_linear:
    a thread adds at most 16 rows."""
    import tile_walk_ref as R
    if case.producer in ("dense_fp32", "gather"):
        return (32 if case.cout > 64 else 16), "fp32", R.DEFAULT_CAPS
    if case.producer == "group_linear":
        return 16, "rows", R.DEFAULT_CAPS
    pooled = case.producer in ("pool", "pieces")
    tiles = 7 if opt(case, "kind") == "device" else case.rows // 128
    cin, cout = (case.cout, C1) if case.producer in DOUBLE_PRODUCERS else (case.cin, case.cout)  # their consumer is the fused GEMM
    variant, gx, ny = R.plan(case.rows, cin, cout, epi_pooled=pooled)
    caps = R.DEFAULT_CAPS
    if case.gx is not None:
        assert variant in ("2x2", "4x1"), "the %s layout cannot be capped" % variant
        caps = (case.gx * ny, R.DEFAULT_CAPS[1]) if variant == "2x2" else (R.DEFAULT_CAPS[0], case.gx * ny)
        variant, gx, ny = R.plan(case.rows, cin, cout, epi_pooled=pooled, cap22=caps[0], cap41=caps[1])
        assert gx == case.gx
    else:
        assert gx == case.rows // 128, "one tile per workgroup expected under the default caps"
    return PER_TILE[variant] * max(R.walk_lengths(tiles, gx, False)), variant, caps
