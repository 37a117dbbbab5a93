"""The detection head of a dataset: heading bins, classes and size templates, carried through the stack as one immutable value.

The reference fixes its head in config.py:2-3 (12 heading bins, 10 size templates, 10 classes: SUN RGB-D) and dataset.py:36-45 (the
templates).  The kernels below the Python layer take nh / ns / nc and the template table as arguments; a HeadConfig is what hands them
the same values everywhere -- the proposal module's last layer, the loss, the decode, the evaluation, the label encoding, the
checkpoint header.  One size template per class (size2class, dataset.py:80-85), so ns == nc.  A net has one head for life
(VoteNetHotPath(device, head=...)); there is no module-level current head."""
import math

import numpy as np

from ._lib import InvalidArgumentError

MAX_BINS = 32  # the kernels' cap on nh, ns and nc (csrc/loss.hip, csrc/monitors, csrc/proposal_supervision: softmax rows in registers)


class HeadConfig:
    """HeadConfig(nh, mean_sizes, class_names=None): nh heading bins; mean_sizes (nc, 3) float, l, w, h as synth.MEAN_SIZES, one
    template per class; class_names: nc strings, or None.  Immutable and hashable; two heads are equal when nh and every template
    bit are (the names are labels, not part of the network)."""
    __slots__ = ("nh", "nc", "class_names", "_sizes", "_f32", "_f64")

    def __init__(self, nh, mean_sizes, class_names=None):
        if isinstance(nh, bool) or not isinstance(nh, (int, np.integer)) or not 1 <= int(nh) <= MAX_BINS:
            raise InvalidArgumentError("HeadConfig: nh must be an integer in [1, %d] (the kernels' cap on heading bins), got %r" % (MAX_BINS, nh))
        try:
            ms = np.array(mean_sizes, dtype=np.float64)
        except (TypeError, ValueError):
            raise InvalidArgumentError("HeadConfig: mean_sizes must be an (nc, 3) array of floats") from None
        if ms.ndim != 2 or ms.shape[1] != 3:
            raise InvalidArgumentError("HeadConfig: mean_sizes must have shape (nc, 3), got %s" % (ms.shape,))
        nc = ms.shape[0]
        if not 1 <= nc <= MAX_BINS:
            raise InvalidArgumentError("HeadConfig: nc = len(mean_sizes) must be in [1, %d] (the kernels' cap on classes and size "
                                       "templates), got %d" % (MAX_BINS, nc))
        bad = [i for i in range(nc) if not all(math.isfinite(v) and v > 0.0 for v in ms[i])]
        if bad:
            raise InvalidArgumentError("HeadConfig: every size template must be finite and > 0; template %d is %s" % (bad[0], ms[bad[0]].tolist()))
        if class_names is not None:
            class_names = tuple(str(c) for c in class_names)
            if len(class_names) != nc:
                raise InvalidArgumentError("HeadConfig: %d class_names for %d classes" % (len(class_names), nc))
        ms = np.ascontiguousarray(ms)
        ms.setflags(write=False)
        f32 = np.ascontiguousarray(ms, dtype=np.float32)
        f32.setflags(write=False)
        set_ = object.__setattr__
        set_(self, "nh", int(nh))
        set_(self, "nc", int(nc))
        set_(self, "class_names", class_names)
        set_(self, "_f64", ms)
        set_(self, "_f32", f32)
        set_(self, "_sizes", ms.tobytes())

    def __setattr__(self, name, value):
        raise AttributeError("HeadConfig is immutable (build another one)")

    def __delattr__(self, name):
        raise AttributeError("HeadConfig is immutable (build another one)")

    def __reduce__(self):
        return (HeadConfig, (self.nh, self._f64.copy(), self.class_names))

    # ---- derived values ---------------------------------------------------------------------------------------------------
    @property
    def ns(self):
        return self.nc

    @property
    def width(self):
        """Columns of proposals_output (model.py:91)."""
        return 5 + 2 * self.nh + 4 * self.ns + self.nc

    @property
    def obj(self):
        return slice(0, 2)

    @property
    def center(self):
        return slice(2, 5)

    @property
    def heading_cls(self):
        return slice(5, 5 + self.nh)

    @property
    def heading_res(self):
        return slice(5 + self.nh, 5 + 2 * self.nh)

    @property
    def size_cls(self):
        return slice(5 + 2 * self.nh, 5 + 2 * self.nh + self.ns)

    @property
    def size_res(self):
        return slice(5 + 2 * self.nh + self.ns, 5 + 2 * self.nh + 4 * self.ns)

    @property
    def sem(self):
        return slice(self.width - self.nc, self.width)

    @property
    def mean_sizes_f64(self):
        """(nc, 3) float64, host, contiguous, read-only."""
        return self._f64

    @property
    def mean_sizes_f32(self):
        """(nc, 3) float32, host, contiguous, read-only: what the decode kernel reads."""
        return self._f32

    mean_sizes = mean_sizes_f64

    @property
    def is_default(self):
        return self == HeadConfig.sunrgbd()

    def __eq__(self, other):
        return isinstance(other, HeadConfig) and self.nh == other.nh and self._sizes == other._sizes

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((self.nh, self._sizes))

    def __repr__(self):
        return "HeadConfig(nh=%d, nc=%d, width=%d%s)" % (self.nh, self.nc, self.width, ", default" if self.is_default else "")

    # ---- constructors -----------------------------------------------------------------------------------------------------
    @staticmethod
    def sunrgbd():
        """The default head, the reference's: 12 heading bins, the ten SUN RGB-D templates (config.py:2-3, dataset.py:36-45)."""
        global _DEFAULT
        if _DEFAULT is None:
            from . import sunrgbd, synth
            names = getattr(sunrgbd, "CLASS_NAMES", None)
            _DEFAULT = HeadConfig(synth.NH, synth.MEAN_SIZES, names if names is not None and len(names) == len(synth.MEAN_SIZES) else None)
        return _DEFAULT

    @staticmethod
    def from_boxes(size, cls, nc, nh, class_names=None):
        """The head whose templates are the per-class mean sizes of a set of ground-truth boxes: size (nbox, 3) l, w, h and cls (nbox)
        as select_boxes / boxes_from_labels return them (device tensors or host arrays).  The means are taken in float64 on the host:
        this runs once per dataset.  A box whose class is outside [0, nc) is left out; a class without a box is an error."""
        def host(a):
            return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        size, cls = host(size).astype(np.float64), host(cls)
        if isinstance(nc, bool) or not isinstance(nc, (int, np.integer)) or not 1 <= int(nc) <= MAX_BINS:
            raise InvalidArgumentError("HeadConfig.from_boxes: nc must be an integer in [1, %d] (the kernels' cap on classes), got %r" % (MAX_BINS, nc))
        if size.ndim != 2 or size.shape[1] != 3 or cls.shape != (size.shape[0],) or cls.dtype.kind not in "iu":
            raise InvalidArgumentError("HeadConfig.from_boxes: size must be (nbox, 3) and cls (nbox) integers, got %s and %s %s"
                                       % (size.shape, cls.shape, cls.dtype))
        mean = np.zeros((int(nc), 3), np.float64)
        for c in range(int(nc)):
            rows = size[cls == c]
            if len(rows) == 0:
                raise InvalidArgumentError("HeadConfig.from_boxes: class %d has no box: its size template cannot be formed" % c)
            mean[c] = rows.mean(0)
        return HeadConfig(nh, mean, class_names)


_DEFAULT = None  # the one cached immutable default (a value, not a setting: nothing can change it)


def resolve(head, nh, ns, nc):
    """The (nh, ns, nc) of a public function that takes both: a head wins over the keywords' values."""
    if head is None:
        return nh, ns, nc
    if not isinstance(head, HeadConfig):
        raise InvalidArgumentError("head must be a HeadConfig, got %r" % type(head).__name__)
    return head.nh, head.ns, head.nc
