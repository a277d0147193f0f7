"""What the GPU tests share to reach the library under test and the device: the one path entry for ulc-codec_amd, the module,
the device, uploads, and the 4-byte-word spec of a guarded arena (tests/guarded_buffers.py).  Every import is lazy, so collecting
the tests needs neither the library nor a GPU."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))


def amd():
    import ulc_amd
    return ulc_amd


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev())


def word(name, n, role, maxn=None, rps=1, align=4):
    """n 32-bit words as a guarded_buffers spec; maxn: the guard covers the largest count any call of the test uses."""
    return dict(name=name, nbytes=4 * n, align=align, role=role, guard=4 * (maxn or n), row=4, rows_per_stream=rps)
