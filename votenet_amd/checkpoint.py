"""Checkpoints of a VoteNetHotPath: save, restore and resume a training run (the reference's ModelSaver / AutoResumeTrainConfig,
run.py:116-125, and SaverRestore for serving, evaluator.py:239-243).

The state carries the reference's variable names (Tensorpack's Conv2D / FullyConnected / BNReLU scopes, TF's Adam slots):

    <layer>/W, <layer>/b                    Conv2D kernel (1, 1, cin, cout) (utils.py:126,152,291), FullyConnected kernel (cin, cout)
                                            (the voting layers voting0..2, model.py:56; the store calls them voting/fc<i>)
    <layer>/bn/gamma, <layer>/bn/beta       BNReLU -> BatchNorm('bn')
    <layer>/bn/mean/EMA, .../variance/EMA   the BatchNorm moving averages (rows 2 and 3 of VoteNetHotPath._ema_state())
    <var>/Adam, <var>/Adam_1                first and second Adam moments, shaped like <var>        (optimizer=True)
    global_step (int64), learning_rate      the optimizer's step count and rate (model.py:241)     (optimizer=True)

tests/golden/votenet_variable_names.txt lists every key with its shape (sa1/conv0/W: 6 input rows, the reference's xyz-as-features; a
model built with point_features = c has 3 + c there, under the same name, and a file of another width is refused).  The rows of every kernel are in the reference's order already
for the modules VoteNetHotPath builds -- [xyz | features] at an SA layer's first conv, [interpolated | points1] at FP, [seeds_xyz |
seeds_points] at voting -- so a kernel is the store's (cin, cout) matrix reshaped, never permuted.

A file is an .npz of numeric arrays plus one JSON header stored as a uint8 array under HEADER_KEY (format version, npoints, NH / NS / NC
of the net's head and, for another head than the default, its size templates mean_sizes; BatchNorm momentum and epsilon, whether
optimizer state is present).  It is read with allow_pickle=False: nothing is unpickled.

A restore copies IN PLACE into the existing store.flat, _ema_flat, _m and _v: a captured StretchGraph has their addresses baked in (its
replay runs votenet_ema_update on them).  Every name, shape, dtype and header field is checked before the first byte is written; then
the derived copies of the parameters (split images, transposes, padded copies, inference BatchNorm tables) are marked stale.  The copies
run on the current stream, so a load between two train_step calls, or before predict, needs no other synchronisation."""
import json
import math
import os

import numpy as np
import torch

FORMAT_VERSION = 1
HEADER_KEY = "__header__"
SA1_FIRST = "sa1/conv0/W"  # (1, 1, 3 + c, 64): the kernel whose input width follows the model's point_features


def _layers(net):
    """(layer, reference scope, FullyConnected?) for every layer, in the order the store declares their tensors."""
    out = []
    for m in (net.sa1, net.sa2, net.sa3, net.sa4, net.fp1, net.fp2):
        out += [(L, L.name, False) for L in m.mlp]
    out += [(L, "voting%d" % i, True) for i, L in enumerate(net.voting)]  # FullyConnected('voting%d'), model.py:56
    out += [(L, L.name, False) for L in net.proposal.mlp + (net.proposal.mlp2 or [])]
    return out


def _entries(net, optimizer=True):
    """[(key, shape, kind, source)] of the model's state in file order.  kind: 'param' (source: the store's tensor name), 'mean' /
    'variance' (source: the layer name), 'adam_m' / 'adam_v' (source: the store's tensor name), 'step', 'lr'."""
    params, ema = [], []
    for L, scope, fc in _layers(net):
        for k in ("W", "b") + (("gamma", "beta") if L.bn else ()):
            name = L.name + "/" + k
            shape = tuple(net.store.views[name].shape)
            if k == "W" and not fc:
                shape = (1, 1) + shape
            params.append((scope + "/" + ("bn/" + k if k in ("gamma", "beta") else k), shape, "param", name))
        if L.bn:
            ema += [(scope + "/bn/mean/EMA", (L.cout,), "mean", L.name), (scope + "/bn/variance/EMA", (L.cout,), "variance", L.name)]
    covered = {e[3] for e in params}
    if covered != set(net.store.views):  # a tensor added to the store without a name here would silently stay out of every file
        raise RuntimeError("checkpoint: store tensors without a reference name: %s" % sorted(set(net.store.views) - covered))
    out = params + ema
    if optimizer:
        for key, shape, _, name in params:
            out += [(key + "/Adam", shape, "adam_m", name), (key + "/Adam_1", shape, "adam_v", name)]
        out += [("global_step", (), "step", None), ("learning_rate", (), "lr", None)]
    return out


def _header(net, optimizer):
    from . import mlp as M
    head = _head_of(net)
    hdr = dict(format="votenet_amd checkpoint", version=FORMAT_VERSION, npoints=[m.npoint for m in (net.sa1, net.sa2, net.sa3, net.sa4)],
               NH=head.nh, NS=head.ns, NC=head.nc, bn_momentum=net.BN_MOMENTUM, bn_epsilon=M.BN_EPS, optimizer=bool(optimizer))
    if not head.is_default:
        # the size templates the network was trained to refine: float64, which JSON's shortest round-trip repr carries exactly
        hdr["mean_sizes"] = head.mean_sizes_f64.tolist()
    return hdr


def _head_of(net):
    """net.head (a net from before heads existed, or a stand-in without one, has the default head)."""
    from .head import HeadConfig
    head = getattr(net, "head", None)
    return head if head is not None else HeadConfig.sunrgbd()


def _header_mean_sizes(hdr, problems):
    """The file's size templates as an (NC, 3) float64 array -- a file without the field has the default head's --, or None with the
    reason appended to problems."""
    from .head import HeadConfig
    ms = hdr.get("mean_sizes")
    if ms is None:
        return HeadConfig.sunrgbd().mean_sizes_f64
    try:
        a = np.array(ms, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None or a.ndim != 2 or a.shape[1] != 3:
        problems.append("header mean_sizes: not an (NC, 3) list of numbers")
        return None
    return a


def _host(buf):
    """A host copy of a device buffer (a copy on the host as well: numpy views of it must not alias a CPU model's live buffer)."""
    return buf.detach().to("cpu", copy=True)


def _slot(buf, view, base):
    """The elements of `buf` at the place `view` occupies inside `base` (the moments share the parameter bucket's layout)."""
    off = view.storage_offset() - base.storage_offset()
    return buf[off:off + view.numel()].view(view.shape)


def state_dict(net, optimizer=True):
    """key -> numpy array (host copies; one device-to-host copy per buffer).  Without an initialised optimizer, optimizer=True gives
    the state of a fresh one: zero moments, step 0, the default rate."""
    from . import model as VM
    st = net.store
    ema = net._ema_state()
    flat, ema_flat = _host(st.flat), _host(net._ema_flat)
    have_opt = hasattr(net, "_seg")
    m = _host(net._m) if optimizer and have_opt else None
    v = _host(net._v) if optimizer and have_opt else None
    out = {}
    for key, shape, kind, src in _entries(net, optimizer):
        if kind == "param":
            out[key] = _slot(flat, st.views[src], st.flat).numpy().reshape(shape)
        elif kind in ("mean", "variance"):
            out[key] = _slot(ema_flat, ema[src][2 if kind == "mean" else 3], net._ema_flat).numpy()
        elif kind in ("adam_m", "adam_v"):
            buf = m if kind == "adam_m" else v
            out[key] = _slot(buf, st.views[src], st.flat).numpy().reshape(shape) if buf is not None else np.zeros(shape, np.float32)
        elif kind == "step":
            out[key] = np.array(net._step if have_opt else 0, dtype=np.int64)
        else:
            out[key] = np.array(net._lr if have_opt else VM.LEARNING_RATE, dtype=np.float64)
    return out


def _as_array(v):
    if isinstance(v, torch.Tensor):
        return v.detach().to("cpu").numpy()
    return np.asarray(v)


def _validate(net, sd, strict, optimizer=None, problems=(), unreadable=()):
    """-> (key -> array, optimizer state present?) or ValueError naming every offending key (and the `problems` found before).
    optimizer=None: present when any of its keys is (then all of them must be).  unreadable: keys of the file whose arrays could not
    be read (reported among the problems already): present, not checked again."""
    problems = list(problems)
    sd = dict(sd)
    sd.update(dict.fromkeys(unreadable))
    full = _entries(net, True)
    opt_keys = {e[0] for e in full if e[2] in ("adam_m", "adam_v", "step", "lr")}
    if optimizer is None:
        optimizer = any(k in sd for k in opt_keys)
    want = [e for e in full if optimizer or e[0] not in opt_keys]
    wanted = {e[0] for e in want}
    missing = [e[0] for e in want if e[0] not in sd]
    if missing:
        problems.append("missing: %s" % ", ".join(missing))
    if strict:
        extra = [k for k in sd if k not in wanted]
        if extra:
            problems.append("unexpected: %s" % ", ".join(sorted(extra)))
    arrays = {}
    for key, shape, kind, _ in want:
        if key not in sd or key in unreadable:
            continue
        try:
            a = _as_array(sd[key])
        except Exception as e:  # (whatever the value is, it is not an array)
            problems.append("%s: not an array (%s)" % (key, e))
            continue
        if key == SA1_FIRST and a.ndim == len(shape) and a.shape[-2] != shape[-2]:
            # the one width that is the model's choice (VoteNetHotPath(point_features=c): 3 + c rows; 0: the coordinates twice, 6)
            problems.append("%s: the checkpoint's sa1 takes %d input rows, this model's takes %d (3 coordinates + the point features: "
                            "VoteNetHotPath(point_features=%d))" % (key, a.shape[-2], shape[-2], getattr(net, "point_features", 0)))
            continue
        if kind == "step":
            ok = a.dtype.kind in "iu" and a.shape == () and int(a) >= 0
            want_s = "a non-negative integer scalar"
        elif kind == "lr":
            ok = a.dtype.kind == "f" and a.shape == () and math.isfinite(float(a)) and float(a) >= 0
            want_s = "a finite non-negative float scalar"
        else:
            ok = a.dtype == np.float32 and a.shape == shape
            want_s = "float32 %s" % (shape,)
        if not ok:
            problems.append("%s: %s %s, expected %s" % (key, a.dtype, a.shape, want_s))
            continue
        arrays[key] = a
    if problems:
        raise ValueError("checkpoint does not fit this VoteNetHotPath (nothing was loaded): " + "; ".join(problems))
    return arrays, optimizer


def _copy_in(buf, parts):
    """Write host arrays into views of `buf` IN PLACE: one copy of buf to the host, the arrays written there, one copy back -- both
    on the current stream.  Elements outside the views (alignment padding, the moving-average blocks' unused rows) keep their values."""
    img = _host(buf)
    for view, a in parts:
        _slot(img, view, buf).copy_(torch.from_numpy(np.ascontiguousarray(a)).view(view.shape))
    buf.copy_(img)


def load_state_dict(net, sd, strict=True):
    """Restore a state_dict() into the live model, in place.  A missing key, an unexpected key (strict=True), a wrong shape or dtype
    raises ValueError naming every offending key, before anything is written.  Without optimizer state the optimizer is reset (zero
    moments, step 0; the model's rate is kept): moments of another trajectory would be wrong for this one."""
    _restore(net, *_validate(net, sd, strict))


def _restore(net, arrays, optimizer):
    from . import model as VM
    st = net.store
    ema = net._ema_state()
    if not hasattr(net, "_seg"):  # (train_step would initialise it -- and zero what is loaded here -- on its first call)
        net.init_optimizer(float(arrays["learning_rate"]) if optimizer else VM.LEARNING_RATE)
    want = _entries(net, optimizer)
    _copy_in(st.flat, [(st.views[src], arrays[key]) for key, _, kind, src in want if kind == "param"])
    _copy_in(net._ema_flat, [(ema[src][2 if kind == "mean" else 3], arrays[key]) for key, _, kind, src in want if kind in ("mean", "variance")])
    if optimizer:
        for buf, which in ((net._m, "adam_m"), (net._v, "adam_v")):
            _copy_in(buf, [(_slot(buf, st.views[src], st.flat), arrays[key]) for key, _, kind, src in want if kind == which])
        net._step = int(arrays["global_step"])
        net._lr = float(arrays["learning_rate"])
    else:
        net._m.zero_()
        net._v.zero_()
        net._step = 0
    st.params_changed()     # images, transposes, padded copies: rebuilt before their next use
    net._ema_version += 1   # inference_bn() rebuilds its tables, and predict() does not warn about untrained moving averages
    if getattr(net, "step_guard", None) is not None:
        net.step_guard.refresh_snapshot()  # (or a bad step after this restore would bring back the averages from before it)


def save(net, path, optimizer=True):
    """Write the state to `path` (exactly that name) through a temporary file in the same directory: an interrupted save leaves the
    previous checkpoint intact."""
    path = os.fspath(path)
    arrays = {HEADER_KEY: np.frombuffer(json.dumps(_header(net, optimizer)).encode(), dtype=np.uint8)}
    arrays.update(state_dict(net, optimizer))
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        np.savez(f, **arrays)
    os.replace(tmp, path)


def _read(path):
    """-> (header dict or None, key -> array, key -> reason it could not be read).  allow_pickle=False: an object array is a
    reason, never unpickled."""
    arrays, bad = {}, {}
    with np.load(os.fspath(path), allow_pickle=False) as z:
        for k in z.files:
            try:
                arrays[k] = z[k]
            except ValueError as e:
                bad[k] = str(e)
    raw = arrays.pop(HEADER_KEY, None)
    hdr = None
    if raw is not None and raw.dtype == np.uint8 and raw.ndim == 1:
        try:
            hdr = json.loads(raw.tobytes().decode())
        except ValueError:
            hdr = None
    return hdr, arrays, bad


def load(net, path, strict=True):
    """Restore a file written by save() (or converted into its layout).  The header must match the model (format version, npoints,
    NH / NS / NC, the size templates mean_sizes by value -- a file without them has the default head's --, BatchNorm momentum and
    epsilon); it says whether the optimizer state is in the file."""
    hdr, arrays, bad = _read(path)
    problems = ["%s: %s" % (k, why) for k, why in sorted(bad.items())]
    if not isinstance(hdr, dict) or not isinstance(hdr.get("version"), int):
        raise ValueError("%s: no votenet_amd checkpoint header (%s)" % (path, HEADER_KEY))
    if hdr["version"] > FORMAT_VERSION:
        raise ValueError("%s: checkpoint format version %d, this code reads up to %d" % (path, hdr["version"], FORMAT_VERSION))
    mine = _header(net, hdr.get("optimizer"))
    for field in ("npoints", "NH", "NS", "NC", "bn_momentum", "bn_epsilon"):
        if hdr.get(field) != mine[field]:
            problems.append("header %s: file %r, model %r" % (field, hdr.get(field), mine[field]))
    theirs, ours = _header_mean_sizes(hdr, problems), _head_of(net).mean_sizes_f64
    if theirs is not None and (theirs.shape != ours.shape or theirs.tobytes() != ours.tobytes()):
        diff = [i for i in range(min(len(theirs), len(ours))) if theirs[i].tobytes() != ours[i].tobytes()]
        problems.append("header mean_sizes: the file's size templates differ from the model's head%s"
                        % (" (first at template %d: file %r, model %r)" % (diff[0], theirs[diff[0]].tolist(), ours[diff[0]].tolist()) if diff
                           else " (%d templates in the file, %d in the model)" % (len(theirs), len(ours))))
    if not isinstance(hdr.get("optimizer"), bool):
        problems.append("header optimizer: %r, expected true / false" % (hdr.get("optimizer"),))
        hdr["optimizer"] = None
    _restore(net, *_validate(net, arrays, strict, hdr["optimizer"], problems, unreadable=bad))


def load_new(cls, path, device, strict=True, **kw):
    """VoteNetHotPath.load(path, device): build a net for the file -- the head from the header's NH and mean_sizes, npoints, and
    point_features from the rows of sa1's first kernel -- and restore the file into it.  kw: further constructor arguments (seed)."""
    from .head import HeadConfig
    hdr, arrays, _ = _read(path)
    if not isinstance(hdr, dict) or not isinstance(hdr.get("version"), int):
        raise ValueError("%s: no votenet_amd checkpoint header (%s)" % (path, HEADER_KEY))
    problems = []
    ms = _header_mean_sizes(hdr, problems)
    if problems:
        raise ValueError("%s: %s" % (path, "; ".join(problems)))
    head = HeadConfig(hdr.get("NH"), ms)
    if hdr.get("NC") != head.nc or hdr.get("NS") != head.ns:
        raise ValueError("%s: header NS / NC %r / %r, but %d size templates" % (path, hdr.get("NS"), hdr.get("NC"), head.nc))
    if "npoints" in hdr:
        kw.setdefault("npoints", tuple(hdr["npoints"]))
    first = arrays.get(SA1_FIRST)
    if first is not None and first.ndim == 4 and first.shape[2] != 6:
        kw.setdefault("point_features", int(first.shape[2]) - 3)
    net = cls(device, head=HeadConfig.sunrgbd() if head.is_default else head, **kw)
    load(net, path, strict)
    return net
