"""A bounded run of the randomised GPU-vs-oracle sweep (tools/fuzz_parity.py): random geometry (BlockSize 256..8192, 1-3
channels, 22-96 kHz), rate-control mode and parameter, signal shape (synthetic mix, white noise, DC offset, impulse
trains, silence, clipping, beyond full scale), loudness down to digital silence, and calls of varying length.  Every
configuration must be bit-exact in encoded bytes, sizes, WindowCtrl, BlockComplexity and decoded PCM."""
import os
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [20261003, 7])
def test_randomised_parity_sweep(seed):
    import fuzz_parity
    n, nblk = fuzz_parity.run(budget=30.0, seed=seed)
    assert n >= 10 and nblk >= 200, f"the sweep covered too little in its time budget: {n} configurations, {nblk} blocks"


def test_randomised_rate_search_sweep():
    """The rate-search corner on its own (third seed): CBR / ABR at 150-700 kbps, three to five calls per encoder (the search
    window and the keys of a block are carried from probe to probe and from pass to pass), half of the signals beyond full
    scale.  Round 4's randomised sweep found two faults of the rate-search window exactly here."""
    import fuzz_parity
    n, nblk = fuzz_parity.run(budget=40.0, seed=3, rate_search=True)
    assert n >= 8 and nblk >= 100, f"the sweep covered too little in its time budget: {n} configurations, {nblk} blocks"


def test_randomised_many_channel_sweep():
    """The sweep over the geometries tests/geometry_axis_testlib.py adds by hand: BlockSize 256 / 512 / 1024 with 4, 7, 8, 16, 17 and
    32 channels - wave selections whose lanes hold keys of many channels, the gap sums up to their channel limit and the first
    counts without them.  The floor is half of what the first run on an MI355X reached in its 20 s: 389 configurations,
    15568 blocks."""
    import fuzz_parity
    n, nblk = fuzz_parity.run(budget=20.0, seed=11, sizes=[256, 512, 1024], chans=[4, 7, 8, 16, 17, 32])
    assert n >= 194 and nblk >= 7784, f"the sweep covered too little in its time budget: {n} configurations, {nblk} blocks"
