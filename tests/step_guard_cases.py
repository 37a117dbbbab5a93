"""The step guard's case table and its numpy restatement, shared by tests/test_step_guard_cpu.py and tests/test_gpu_step_guard.py (as
tests/loss_cases.py is for the loss): the synthetic bucket, where and with what a gradient is poisoned, the verdict (any non-finite
partial sum of squares, seg_sumsq_kernel's slices) and the counter rules."""
import numpy as np

SLICES, BLOCK = 32, 256          # VOTENET_SUMSQ_SLICES, seg_sumsq_kernel's workgroup
SWEEP = SLICES * BLOCK * 4       # 32 768: one iteration of its unrolled loop over a tensor
# one element; a partial slice; one element past a sweep (the unrolled loop once, then one tail element); four sweeps + an 8 928 tail
LENS = (1, 257, SWEEP + 1, 4 * SWEEP + 8928)
GAPS = (3, 5, 2, 7, 6)           # floats before / between / behind the tensors: the segments start off every alignment
GRAD_STD = (40.0, 1.0, 1000.0, 1.0)  # average norms ||g|| / numel: 40, ~0.06, ~5.5, ~0.003 -> tensors 0, 2 above the clip 0.5, 1, 3 below
CLIP = 0.5
STEPS_SCALES = ((1, 1.0), (7, 0.125))

# where the poisoned element sits: name -> (tensor, offset in the tensor)
POSITIONS = {
    "first_of_tensor0": (0, 0),                    # == the single element of the 1-float tensor
    "partial_slice": (1, 256),                     # the last element of the 257-float tensor: slice 1 holds one element
    "one_past_a_sweep": (2, SWEEP),                # tensor 2's tail loop
    "unrolled_third_accumulator": (3, 50000),      # sweep 1, 17 232 into it: the s2 accumulator of the unrolled loop
    "tail_region": (3, 4 * SWEEP + 4000),
    "last_of_tensor3": (3, LENS[3] - 1),
}
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "overflow_3e19": 3e19}  # 3e19 is finite; its square is not
BAD_CASES = [(p, v) for p in POSITIONS for v in VALUES]


def segments():
    seg, o = [], 0
    for gap, n in zip(GAPS, LENS):
        o += gap
        seg.append((o, o + n))
        o += n
    return seg, o + GAPS[-1]


def bucket(seed=0):
    """-> dict of float32 arrays p, g, m, v over the whole bucket and seg [(a, b)].  The padding between the segments holds NaN in
    every buffer (the optimizer must neither read it into the verdict nor write it); p, m and v carry a -0.0 and a denormal in every
    tensor that has room (a rewrite x = x + 0 or a flush would change their bits)."""
    seg, total = segments()
    rng = np.random.default_rng(seed)
    out = {k: np.full(total, np.nan, np.float32) for k in "pgmv"}
    for (a, b), std in zip(seg, GRAD_STD):
        n = b - a
        out["p"][a:b] = rng.standard_normal(n)
        out["g"][a:b] = rng.standard_normal(n) * std
        out["m"][a:b] = rng.standard_normal(n) * 0.1
        out["v"][a:b] = rng.random(n) * 0.01
        for k in "pmv":
            out[k][a] = -0.0
            if n > 1:
                out[k][b - 1] = 1e-41 if k == "v" else -1e-41
    if abs(out["g"][seg[0][0]]) < 10.0:  # the one-element tensor: its average norm is its magnitude
        out["g"][seg[0][0]] = 40.0
    return out, seg


def poisoned(g, seg, position, value):
    t, off = POSITIONS[position]
    g = g.copy()
    g[seg[t][0] + off] = np.float32(VALUES[value])
    return g


def partial_sums(g, seg):
    """(ntensors, 32) float32: seg_sumsq_kernel's partials -- slice s of a tensor holds its elements i with (i // 256) % 32 == s.
    (Summed in numpy's order, not the kernel's: the verdict asks only whether a partial is finite, and no case here sits at the
    edge of fp32's range.)"""
    out = np.zeros((len(seg), SLICES), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for t, (a, b) in enumerate(seg):
            x = g[a:b].astype(np.float32)
            sl = (np.arange(b - a) // BLOCK) % SLICES
            sq = x * x
            for s in range(SLICES):
                out[t, s] = sq[sl == s].sum(dtype=np.float32)
    return out


def verdict(g, seg):
    """True: a bad step."""
    return not np.isfinite(partial_sums(g, seg)).all()


def average_norms(g, seg, scale):
    return [float(np.sqrt((g[a:b].astype(np.float64) ** 2).sum()) * scale / (b - a)) for a, b in seg]
