"""Oracle references of the clip-spectra tests (tests/test_clip_spectra_capi.py, tests/test_gpu_clip_spectra.py,
tests/test_gpu_clip_spectra_paths.py): what ulcx_analyse_clips_* and ulcx_encode_clips_spectra_* must give for a row - the
coefficients the oracle's encoder holds in TransformBuffer after every block of the clip (oracle_encode_debug's `coef`), its
WindowCtrl (`wc`) and BlockComplexity (`cplx`), channels-first and zero behind the clip's last block.  The oracle run is that of
clips_testlib.ClipRef: the clip interleaved into nb * BlockSize samples, then zeros, from a fresh state.  The waves, cases and
geometries are clips_testlib's; LR is spectra_testlib.to_lr of the oracle's planes.  CPU only."""
import functools
import numpy as np
import clips_testlib as ct
from ulc_testlib import oracle_encode_debug
from spectra_testlib import to_lr, same_bits
from rates_testlib import mode_of

SPECTRA_LR = 1
DEPTHS = (8, 5, 11)                                        # nBlocks of the short case: exact; cuts rows 5 and 6 inside a chunk; three planes behind the last chunk


class SpecRef:
    """One clip from the oracle alone: coef [nb][ch][bs], wc [nb], cplx [nb]."""

    def __init__(self, bs, ch, clip):
        L = clip.shape[1]
        self.bs, self.ch, self.L, self.nb = bs, ch, L, ct.clip_blocks(bs, L)
        self.coef, self.wc, self.cplx = np.zeros((self.nb, ch, bs), np.float32), np.zeros(self.nb, np.int32), np.zeros(self.nb, np.float32)
        if self.nb:
            pcm = np.zeros((self.nb * bs, ch), np.float32)
            pcm[:L] = clip.T
            mode, p0, p1 = mode_of(ct.SCALAR)
            r = oracle_encode_debug(pcm, bs, ct.RATE, mode, p0, p1, slot=2 * ch * bs + 16)
            self.coef, self.wc, self.cplx = r["coef"].reshape(self.nb, ch, bs), r["wc"], r["cplx"]


@functools.lru_cache(maxsize=None)
def row_spec(bs, ch, i, case=None):
    """Pair i's reference (shared by the tests that use it; nobody writes to it)."""
    case = case or ct.short_case(bs)
    return SpecRef(bs, ch, ct.wave(bs, ch, case.T)[i][:, :case.lengths[i]])


def specs(bs, ch, case=None, rows=None):
    return [row_spec(bs, ch, i % 7, case) for i in (range(7) if rows is None else rows)]


def expected(refs, n_blocks, lr=False):
    """-> (coef [n][ch][n_blocks][bs], wc [n][n_blocks], cplx [n][n_blocks]) of the rows `refs`: block k of a row is live when
    k < min(n_blocks, nb); everything else is +0."""
    n, ch, bs = len(refs), refs[0].ch, refs[0].bs
    coef, wc, cplx = np.zeros((n, ch, n_blocks, bs), np.float32), np.zeros((n, n_blocks), np.int32), np.zeros((n, n_blocks), np.float32)
    for i, r in enumerate(refs):
        m = min(n_blocks, r.nb)
        coef[i, :, :m] = r.coef[:m].transpose(1, 0, 2)
        wc[i, :m], cplx[i, :m] = r.wc[:m], r.cplx[:m]
    return (to_lr(coef) if lr else coef), wc, cplx


def check_planes(got_coef, got_wc, got_cplx, refs, n_blocks, lr, what):
    """The call's planes against the oracle's, bit for bit; got_wc / got_cplx None: not asked for."""
    coef, wc, cplx = expected(refs, n_blocks, lr)
    assert got_coef.shape == coef.shape, (what, got_coef.shape, coef.shape)
    if not same_bits(got_coef, coef):
        bad = np.argwhere(got_coef.view(np.uint32) != coef.view(np.uint32))
        i, c, k, j = bad[0]
        raise AssertionError(f"{what}: {len(bad)} coefficients differ from the oracle's, first at row {i} (of {refs[i].nb} blocks) channel {c} block {k} "
                             f"bin {j}: {got_coef[i, c, k, j]!r} vs {coef[i, c, k, j]!r}; last at {bad[-1].tolist()}")
    if got_wc is not None:
        assert np.array_equal(got_wc, wc), f"{what}: window codes {got_wc.tolist()} vs the oracle's {wc.tolist()}"
    if got_cplx is not None:
        assert same_bits(got_cplx, cplx), f"{what}: complexities differ from the oracle's at {np.argwhere(got_cplx.view(np.uint32) != cplx.view(np.uint32)).tolist()[:8]}"
