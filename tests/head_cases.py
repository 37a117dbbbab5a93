"""The detection heads the head tests use (tests/test_head_cpu.py, tests/test_gpu_head.py).  Each is chosen for the path the proposal
module's last layer takes -- pointnet2.Layer runs a plain layer whose width is no multiple of 64 on copies padded to the next one --
and for a kernel edge:

    scannet    nh 1,  nc 18, width 97   one heading bin (a softmax over one logit; floormod(res * pi, 2 pi) in decode); padded to 128
    tiny       nh 2,  nc 3,  width 24   narrower than one 64-column tile; padded to 64
    exact64    nh 2,  nc 11, width 64   a plain last layer that IS a multiple of 64: the unpadded route
    exact128   nh 4,  nc 23, width 128  the same route at the width of the default head's padded copy
    wide       nh 12, nc 32, width 189  above 128, padded to 192; nc at the kernels' cap
    default    nh 12, nc 10, width 79   passed explicitly; must equal the implicit one
"""
HEADS = dict(scannet=(1, 18), tiny=(2, 3), exact64=(2, 11), exact128=(4, 23), wide=(12, 32), default=(12, 10))
WIDTH_PAD = dict(scannet=(97, 128), tiny=(24, 64), exact64=(64, 0), exact128=(128, 0), wide=(189, 192), default=(79, 128))  # width, Layer.cout_pad


def head(name):
    from votenet_amd import synth
    return synth.room_head(*HEADS[name])
