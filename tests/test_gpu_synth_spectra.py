"""Synthesis from spectra on the GPU (include/ulc_amd.h section 3: ulcx_synth_spectra_*): PCM from caller-held MDCT planes through
the decoder's inverse transform.  Expectations never come from this library's own decode: planes, codes and PCM of a stream are
the two sides of ONE oracle run (tests/synth_spectra_testlib.py, orc_decode_stream_coefs) and are compared bit for bit (uint32 /
int16 views); arbitrary planes are compared with the float64 referee (tests/mdct_referee.py) at the project's TOL.  What the inputs
hold is asserted without a GPU in tests/test_synth_spectra_capi.py.  Outputs are poisoned before every call."""
import numpy as np
import pytest

from gpu_testlib import amd as _amd
import guarded_buffers as gb
import mdct_referee as R
import synth_spectra_testlib as Y
from seek_testlib import geometries

pytestmark = pytest.mark.gpu
GEOMS = sorted(geometries().keys())
LR, WARM = Y.SPECTRA_LR, Y.SYNTH_WARM
N = Y.N_OUT
ERR_ARG = -1


def synth(dec, coef, wc, flags, pcm16=False):
    """One ulcx_synth_spectra_dev(_pcm16) call on poisoned outputs -> (pcm [n][C][nOut * bs], live [n][nOut]) as numpy."""
    import torch
    n, ch, npl, bs = coef.shape
    n_out = npl - (1 if flags & WARM else 0)
    d_coef = torch.from_numpy(np.ascontiguousarray(coef, np.float32)).to("cuda:0")
    d_wc = torch.from_numpy(np.ascontiguousarray(wc, np.int32)).to("cuda:0")
    pcm = torch.full((n, ch, n_out * bs), int(Y.POISON_I16) if pcm16 else float(Y.POISON_F), dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
    live = torch.full((n, n_out), int(Y.POISON_I32), dtype=torch.int32, device="cuda:0")
    dec.synth_spectra_dev(n, npl, flags, d_coef.data_ptr(), d_wc.data_ptr(), pcm.data_ptr(), live.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    assert same(d_coef.cpu().numpy(), np.ascontiguousarray(coef, np.float32)) and same(d_wc.cpu().numpy(), np.ascontiguousarray(wc, np.int32))   # the inputs stay
    return pcm.cpu().numpy(), live.cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_rows(got, want, bs, what):
    """PCM and live of every row, bit for bit; the first row that differs is named with the block and channel."""
    (pcm, live), (wpcm, wlive) = got, want
    assert pcm.shape == wpcm.shape and pcm.dtype == wpcm.dtype, (pcm.shape, wpcm.shape, pcm.dtype)
    for i in range(wpcm.shape[0]):
        assert np.array_equal(live[i], wlive[i]), f"{what}: row {i}: live {live[i]} vs {wlive[i]}"
        if not same(pcm[i], wpcm[i]):
            bad = np.argwhere(pcm[i] != wpcm[i]) if pcm.dtype == np.int16 else np.argwhere(pcm[i].view(np.uint32) != wpcm[i].view(np.uint32))
            blocks = sorted({int(t) // bs for _, t in bad})
            raise AssertionError(f"{what}: row {i}: {len(bad)} of {wpcm[i].size} samples differ, first at (channel, t) = {bad[0].tolist()}, "
                                 f"output blocks {blocks}")


def check_both_forms(dec, coef, wc, pcm, live, flags, bs, what):
    check_rows(synth(dec, coef, wc, flags), (pcm, live), bs, f"{what}, float")
    check_rows(synth(dec, coef, wc, flags, pcm16=True), (Y.to_pcm16(pcm), live), bs, f"{what}, pcm16")


# ---------------------------------------------------------------------------------------------------------------------
# 1. decoded planes give the decoder's PCM
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_decoded_planes_give_the_decoders_pcm(geom):
    """70 rows per call, float and PCM16: with the plane in front, rows that start at block 1, directly behind window-switched
    blocks, near and past the stream's end (codes ending in 0) and at seeded blocks; without it, rows from block 0 that end at
    every plane.  2048 x 2 and 4096 x 2 run k_dsyn's two constants paths, 1 / 3 / 6 channels k_dgen."""
    bs, ch = geom
    refs = Y.geom_streams(geom)
    dec = _amd().BatchDecoder(70, ch, bs, N + 1)
    coef, wc, pcm, live = Y.stack(refs, Y.warm_rows(refs), N, 1)
    check_both_forms(dec, coef, wc, pcm, live, WARM, bs, f"{bs}x{ch} warm")
    assert live.sum() >= 250 and (live == 0).sum() >= 20 and pcm.any()
    coef, wc, pcm, live = Y.head_rows(refs)
    check_both_forms(dec, coef, wc, pcm, live, 0, bs, f"{bs}x{ch} from block 0")
    dec.close()


def test_three_blocks_at_32768():
    ref = Y.big_ref()
    dec = _amd().BatchDecoder(2, 1, ref.bs, 4)
    coef, wc, pcm, live = Y.stack([ref], [(0, 0)], 3, 0)
    check_both_forms(dec, coef, wc, pcm, live, 0, ref.bs, "32768x1 from block 0")
    coef, wc, pcm, live = Y.stack([ref], [(0, 1), (0, 2)], 2, 1)
    check_both_forms(dec, coef, wc, pcm, live, WARM, ref.bs, "32768x1 warm")
    assert live.tolist() == [[1, 1], [1, 0]]
    dec.close()


@pytest.mark.parametrize("geom", [(2048, 2), (4096, 2)])
def test_whole_rows_across_the_chunk_tables(geom, monkeypatch):
    """One workgroup per row (no cut) over 39 blocks: the stereo kernel restages its per-chunk window codes inside the row."""
    monkeypatch.setenv("ULCX_DSYN_SPLIT", "0")
    bs, ch = geom
    ref = Y.geom_streams(geom)[0]
    assert ref.K == 40
    dec = _amd().BatchDecoder(2, ch, bs, 40)
    coef, wc, pcm, live = Y.stack([ref], [(0, 1), (0, 3)], 39, 1)
    check_rows(synth(dec, coef, wc, WARM), (pcm, live), bs, f"{bs}x{ch} 39 blocks")
    assert dec.last_cut()[0] == 0 and live[0].all() and live[1].sum() == 37
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. every header code
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(256, 1), (2048, 2), (4096, 2)])
def test_every_header_code(geom):
    bs, ch = geom
    ref = Y.code_stream(bs, ch)
    firsts = Y.windows(ref.K, 8)
    dec = _amd().BatchDecoder(len(firsts), ch, bs, 9)
    coef, wc, pcm, live = Y.stack([ref], [(0, f) for f in firsts], 8, 1)
    assert {int(w) for w in wc[:, 1:].ravel() if w} == {int(w) for w in ref.wc[1:]}
    check_both_forms(dec, coef, wc, pcm, live, WARM, bs, f"every code {bs}x{ch} warm")
    coef, wc, pcm, live = Y.stack([ref], [(0, 0)], 8, 0)
    check_both_forms(dec, coef, wc, pcm, live, 0, bs, f"every code {bs}x{ch} from block 0")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. ULCX_SPECTRA_LR
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (2048, 3), (1024, 6)])
def test_lr_skips_the_unmix(geom):
    """The coded mid / side planes passed under LR come out un-mixed per channel: float32 a + b and a - b of a pair, formed in numpy,
    are the oracle's PCM bit for bit, and a trailing single channel is the oracle's directly."""
    bs, ch = geom
    refs = Y.geom_streams(geom)
    rows = Y.warm_rows(refs, total=24)
    dec = _amd().BatchDecoder(len(rows), ch, bs, N + 1)
    coef, wc, pcm, live = Y.stack(refs, rows, N, 1)
    got, glive = synth(dec, coef, wc, WARM | LR)
    dec.close()
    assert np.array_equal(glive, live)
    mixed = got.copy()
    for c in range(0, ch - 1, 2):
        mixed[:, c], mixed[:, c + 1] = got[:, c] + got[:, c + 1], got[:, c] - got[:, c + 1]
    check_rows((mixed, glive), (pcm, live), bs, f"{bs}x{ch} LR, re-mixed in numpy")
    assert not same(got[:, 0], pcm[:, 0])                   # (it did skip something)


def test_lr_on_stereo_below_2048():
    """Stereo below BlockSize 2048 takes the two-wave synthesis with the BlockSize read at run time, which no geometry above has
    under LR: rows of 4 blocks over every header code of a 256 x 2 stream (every decimated tail), with the plane in front and
    from block 0, float and PCM16 - the coded planes give the oracle's PCM, and under LR its re-mix in numpy, bit for bit."""
    bs, ch, n_out = 256, 2, 4
    ref = Y.code_stream(bs, ch)
    dec = _amd().BatchDecoder(len(Y.windows(ref.K, n_out)), ch, bs, n_out + 1)
    for rows, warm in (([(0, f) for f in Y.windows(ref.K, n_out)], 1), ([(0, 0)], 0)):
        coef, wc, pcm, live = Y.stack([ref], rows, n_out, warm)
        assert any(int(w) != 0x10 for w in wc[:, warm:].ravel() if w)
        check_both_forms(dec, coef, wc, pcm, live, WARM * warm, bs, f"{bs}x{ch} warm {warm}")
        for pcm16 in (False, True):
            got, glive = synth(dec, coef, wc, WARM * warm | LR, pcm16=pcm16)
            if pcm16:                                       # (the conversion clamps: PCM16 under LR is the conversion of the float planes)
                check_rows((got, glive), (Y.to_pcm16(lr_f), live), bs, f"{bs}x{ch} warm {warm} LR, pcm16")
                continue
            lr_f = got
            mixed = np.stack([got[:, 0] + got[:, 1], got[:, 0] - got[:, 1]], axis=1)
            check_rows((mixed, glive), (pcm, live), bs, f"{bs}x{ch} warm {warm} LR, re-mixed in numpy")
            assert not same(got[:, 0], pcm[:, 0])
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. arbitrary planes against the float64 referee
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, LR], ids=["ms", "lr"])
@pytest.mark.parametrize("geom", [(2048, 2), (4096, 2), (256, 6), (32768, 1)])
def test_arbitrary_planes_match_the_referee(geom, flags):
    """Seeded normal coefficients under a seeded sequence of every header code, three all-zero blocks in the middle: every (row,
    channel, block) unit within TOL = 1e-5 of the unit's peak of the float64 referee (tests/mdct_referee.py), all-zero units exact
    zeros.  Rows with the plane in front that cover blocks 1 .. K - 1, and the row from block 0.
    Worst unit error measured on an MI355X: 2.2e-7 .. 2.6e-7 of the peak at every shape, flags 0 and LR (profiles/synth_spectra_bench.txt)."""
    bs, ch = geom
    case = Y.referee_case(bs, ch, seed=bs + ch)
    key = "lr" if flags & LR else "ms"
    n_out = 8
    coef, wc, want, live = Y.case_rows(case, n_out, 1, key)
    dec = _amd().BatchDecoder(len(coef), ch, bs, n_out + 1)
    got, glive = synth(dec, coef, wc, flags | WARM)
    assert np.array_equal(glive, live)
    e = R.unit_errors(Y.unit_rows(got, bs), Y.unit_rows(want, bs))
    coef0, wc0, want0, live0 = Y.case_rows(case, n_out, 0, key)
    got0, glive0 = synth(dec, coef0, wc0, flags)
    dec.close()
    assert np.array_equal(glive0, live0)
    e0 = R.unit_errors(Y.unit_rows(got0, bs), Y.unit_rows(want0, bs))
    zero_units = int((np.abs(Y.unit_rows(want, bs)).max(axis=-1) == 0).sum())
    print(f"{bs}x{ch} flags {flags}: worst unit error {max(e.max(), e0.max()):.3e} of the peak ({e.size + e0.size} units, {zero_units} all-zero)")
    assert zero_units >= 2 * ch
    assert max(e.max(), e0.max()) <= Y.TOL, (np.unravel_index(e.argmax(), e.shape), e.max(), e0.max())


# ---------------------------------------------------------------------------------------------------------------------
# 5. row ends and untrusted codes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (4096, 2), (1024, 6)])
def test_bad_codes_end_their_row_only(geom):
    """0, 0x05, 0x25, 0x100, -1 and 0x7FFFFFFF at the first, a middle and the last plane and at the plane in front: zeros and live 0
    from there on (the whole row for the plane in front), and the rows beside them bit-exact."""
    bs, ch = geom
    refs = Y.geom_streams(geom)
    base = Y.warm_rows(refs, total=12)[:2] + [(0, 7), (0, 11)]
    rows, plant = [], []
    for j, code in enumerate(Y.BAD_CODES):
        for at in (0, 1, 3, N):                             # plane in front, first, middle, last output plane
            rows += [base[(j + at) % len(base)], base[(j + at + 1) % len(base)]]
            plant += [(code, at), None]
    coef, wc, pcm, live = Y.stack(refs, rows, N, 1)
    coef, wc, pcm, live = coef.copy(), wc.copy(), pcm.copy(), live.copy()
    for i, p in enumerate(plant):
        if p is not None and live[i].all():
            code, at = p
            wc[i, at] = code
            t = max(at - 1, 0)
            pcm[i, :, t * bs:] = 0
            live[i, t:] = 0
    assert sum(p is not None for p in plant) == 24 and (live.sum(axis=1) == N).sum() >= 20
    dec = _amd().BatchDecoder(len(rows), ch, bs, N + 1)
    check_both_forms(dec, coef, wc, pcm, live, WARM, bs, f"{bs}x{ch} bad codes")
    dec.close()


@pytest.mark.parametrize("geom", [(2048, 2), (1024, 6)])
def test_nan_and_inf_stay_in_two_blocks(geom):
    """A NaN and an Inf in one plane each: only that block and its successor differ, in that row only."""
    bs, ch = geom
    refs = Y.geom_streams(geom)
    rows = [(0, 5), (0, 5), (0, 5), (0, 9)]
    coef, wc, pcm, live = Y.stack(refs, rows, N, 1)
    coef = coef.copy()
    coef[1, 0, 2, 17] = np.nan                              # plane 2 = output block 1 of row 1
    coef[2, ch - 1, 3, bs - 1] = np.inf
    dec = _amd().BatchDecoder(len(rows), ch, bs, N + 1)
    got, glive = synth(dec, coef, wc, WARM)
    dec.close()
    assert np.array_equal(glive, live)
    check_rows((got[[0, 3]], glive[[0, 3]]), (pcm[[0, 3]], live[[0, 3]]), bs, "rows beside")
    for i, blk in ((1, 1), (2, 2)):
        g, w = Y.unit_rows(got[i:i + 1], bs)[0], Y.unit_rows(pcm[i:i + 1], bs)[0]
        for k in range(N):
            if k not in (blk, blk + 1):
                assert same(g[:, k], w[:, k]), f"row {i}: block {k} differs although the bad value sits in plane {blk + 1}"
        # (a coefficient of a decimated block's late sub-block reaches the output only with the next block: either of the two)
        assert not np.isfinite(g[:, blk:blk + 2]).all(), i
    assert not np.isfinite(Y.unit_rows(got[1:2], bs)[0][:, 1]).all()      # coefficient 17 sits in the block's first sub-block


# ---------------------------------------------------------------------------------------------------------------------
# 6. the even cut
# ---------------------------------------------------------------------------------------------------------------------
def test_few_long_rows_are_cut_evenly():
    bs, ch = 2048, 2
    refs = Y.geom_streams((bs, ch))
    assert refs[0].K == 40
    dec = _amd().BatchDecoder(2, ch, bs, 41)
    coef, wc, pcm, live = Y.head_rows(refs[:1], n_out=40, total=1)
    coef, wc, pcm, live = (np.concatenate([a, a]) for a in (coef, wc, pcm, live))
    got = synth(dec, coef, wc, 0)
    cut = dec.last_cut()
    assert cut[0] > 2 and cut[1] == 0, cut                  # more workgroups than rows: the rows were cut
    check_rows(got, (pcm, live), bs, "2 x 40 blocks, cut")
    coef, wc, pcm, live = Y.stack(refs[:1], [(0, 1), (0, 2)], 39, 1)
    got = synth(dec, coef, wc, WARM, pcm16=True)
    assert dec.last_cut()[0] > 2
    check_rows(got, (Y.to_pcm16(pcm), live), bs, "2 x 39 blocks warm, cut, pcm16")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. clean planes: analysis, then synthesis
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr", [False, True], ids=["ms", "lr"])
@pytest.mark.parametrize("geom", [(2048, 2), (4096, 2)])
def test_clean_planes_round_trip(geom, lr):
    """ulcx_analyse_clips_dev's planes and codes through the synthesis: the input delayed by 2 * BlockSize, every (channel, block)
    unit within TOL of its peak - with transients, so the codes switch windows.  Measured on an MI355X: 3.7e-7 .. 4.5e-7."""
    import torch
    import corpus
    from test_transform_referee import transient_pcm
    amd = _amd()
    bs, ch = geom
    K, n = 12, 3
    x = np.stack([transient_pcm(bs, K, ch, seed=31 + i) for i in range(n)])                 # [n][K bs][C]
    wave = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to("cuda:0")
    enc = amd.BatchEncoder(n, ch, bs, 44100, K + 2)
    coef, wc, _ = corpus.clip_spectra(enc, wave, lr=lr)
    assert coef.shape[2] == K + 2
    dec = amd.BatchDecoder(n, ch, bs, K + 3)
    pcm, live = corpus.synth_spectra(dec, coef, wc, lr=lr)
    torch.cuda.synchronize()
    codes = wc.cpu().numpy()
    assert live.cpu().numpy().all() and len({int(w) for w in codes.ravel()}) >= 3
    got = pcm.cpu().numpy()[:, :, 2 * bs:]                                                     # [n][C][K bs]
    e = R.unit_errors(Y.unit_rows(got, bs), Y.unit_rows(np.ascontiguousarray(x.transpose(0, 2, 1)), bs))
    print(f"{bs}x{ch} lr={lr}: worst unit error {e.max():.3e} of the peak")
    enc.close(); dec.close()
    assert e.max() <= Y.TOL, (np.unravel_index(e.argmax(), e.shape), e.max())


# ---------------------------------------------------------------------------------------------------------------------
# 8. state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (1024, 1)])
def test_no_stream_state_moves(geom):
    """A streaming decode split around a synth call equals the oracle's unsplit one; a sample crop behind a synth call is the oracle's."""
    from test_gpu_crops import _geom_corpus
    from test_gpu_sample_crops import _device_samples, _check_rows
    bs, ch = geom
    name, blocks, bits, _ = geometries()[geom][0]
    ref = Y.geom_streams(geom)[0]
    K = 12
    dec = _amd().BatchDecoder(2, ch, bs, K)
    two = np.stack([blocks[:K], blocks[K:2 * K]])
    a, _ = dec.decode(two[:, :5])
    coef, wc, pcm, live = Y.stack([ref], [(0, 3), (0, 20)], N, 1)
    check_rows(synth(dec, coef, wc, WARM), (pcm, live), bs, "between two decode calls")
    b, _ = dec.decode(two[:, 5:])
    whole = np.concatenate([a, b], axis=1)                  # [2][K bs][C]
    assert same(whole[0].T, Y.pcm_planes(ref)[:, :K * bs]), "stream 0 differs from the unsplit decode"
    cor = _geom_corpus(geom)
    files, start, ns = [0, 0], [3 * bs + 17, 0], 2 * bs + 5
    check_rows(synth(dec, coef, wc, WARM), (pcm, live), bs, "in front of a sample crop")
    got, gbits = _device_samples(dec, cor, files, start, ns)
    _check_rows(cor, files, start, ns, got, gbits, "behind a synth call")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals before any device work
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_poisoned():
    import torch
    amd = _amd()
    bs, ch, B, maxK = 256, 2, 4, 6
    dec = amd.BatchDecoder(B, ch, bs, maxK)
    coef = torch.zeros((B, ch, maxK, bs), dtype=torch.float32, device="cuda:0")
    wc = torch.full((B, maxK), 0x10, dtype=torch.int32, device="cuda:0")
    pcm = torch.full((B * ch * maxK * bs + 8,), float(Y.POISON_F), dtype=torch.float32, device="cuda:0")
    pcm16 = torch.full((B * ch * maxK * bs + 8,), int(Y.POISON_I16), dtype=torch.int16, device="cuda:0")
    live = torch.full((B * maxK + 8,), int(Y.POISON_I32), dtype=torch.int32, device="cuda:0")
    l = amd.lib()
    good = dict(n=B, nb=3, flags=0, coef=coef.data_ptr(), wc=wc.data_ptr(), pcm=pcm.data_ptr(), live=live.data_ptr())
    cases = [dict(n=0), dict(n=-1), dict(n=B + 1), dict(nb=0), dict(nb=maxK), dict(nb=1, flags=WARM), dict(nb=0, flags=WARM), dict(nb=maxK + 1, flags=WARM),
             dict(flags=4), dict(flags=WARM | LR | 8), dict(flags=-1), dict(coef=0), dict(wc=0), dict(pcm=0), dict(live=0),
             dict(coef=coef.data_ptr() + 4), dict(coef=coef.data_ptr() + 8), dict(wc=wc.data_ptr() + 2), dict(pcm=pcm.data_ptr() + 4), dict(pcm=pcm.data_ptr() + 8),
             dict(live=live.data_ptr() + 1), dict(live=live.data_ptr() + 2)]
    for c in cases:
        a = dict(good, **c)
        rc = l.ulcx_synth_spectra_dev(dec.h, a["n"], a["nb"], a["flags"], a["coef"], a["wc"], a["pcm"] or None, a["live"] or None, None)
        assert rc == ERR_ARG, (c, rc)
        assert b"ulcx_synth_spectra_dev:" in l.ulcx_last_error() or b"not aligned" in l.ulcx_last_error()
    good16 = dict(good, pcm=pcm16.data_ptr())
    for c in (dict(pcm=pcm16.data_ptr() + 2), dict(pcm=pcm16.data_ptr() + 1), dict(pcm=0), dict(nb=maxK), dict(flags=16), dict(n=B + 1)):
        a = dict(good16, **c)
        assert l.ulcx_synth_spectra_dev_pcm16(dec.h, a["n"], a["nb"], a["flags"], a["coef"], a["wc"], a["pcm"] or None, a["live"], None) == ERR_ARG, c
    torch.cuda.synchronize()
    assert bool((pcm == float(Y.POISON_F)).all()) and bool((pcm16 == int(Y.POISON_I16)).all()) and bool((live == int(Y.POISON_I32)).all())
    # the widest calls the object takes are taken: maxBlocksPerCall - 1 output blocks, with and without the plane in front
    for nb, flags in ((maxK - 1, 0), (maxK, WARM)):
        assert l.ulcx_synth_spectra_dev(dec.h, B, nb, flags, coef.data_ptr(), wc.data_ptr(), pcm.data_ptr(), live.data_ptr(), None) == 0
        torch.cuda.synchronize()
        n_out = maxK - 1
        assert bool((pcm[:B * ch * n_out * bs] == 0).all()) and bool((pcm[B * ch * n_out * bs:] == float(Y.POISON_F)).all())
        assert bool((live[:B * n_out] == 1).all()) and bool((live[B * n_out:] == int(Y.POISON_I32)).all())
        pcm.fill_(float(Y.POISON_F)); live.fill_(int(Y.POISON_I32))
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. host form, guards, binding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (2048, 3)])
def test_host_form_equals_the_device_form(geom):
    bs, ch = geom
    refs = Y.geom_streams(geom)
    rows = Y.warm_rows(refs, total=9)
    dec = _amd().BatchDecoder(len(rows), ch, bs, N + 1)
    for flags in (WARM, WARM | LR, 0):
        coef, wc, pcm, live = Y.stack(refs, rows, N, 1) if flags & WARM else Y.head_rows(refs, total=9)
        hp, hl = dec.synth_spectra(coef, wc, flags)
        dp, dl = synth(dec, coef, wc, flags)
        assert same(hp, dp) and np.array_equal(hl, dl), flags
        if not flags & LR:
            check_rows((hp, hl), (pcm, live), bs, f"host form, flags {flags}")
    dec.close()


@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
@pytest.mark.parametrize("geom", [(2048, 2), (1024, 6)])
def test_nothing_outside_the_outputs_is_written(geom, pcm16):
    """One call with every buffer carved from a poisoned arena between guards, each at an odd multiple of the alignment the header
    states: nothing outside d_pcm / d_live is written, d_coef and d_wc stay as loaded, the outputs are the oracle's."""
    import torch
    bs, ch = geom
    refs = Y.geom_streams(geom)
    rows = Y.warm_rows(refs, total=10)
    n = len(rows)
    coef, wc, pcm, live = Y.stack(refs, rows, N, 1)
    el = 2 if pcm16 else 4
    specs = [dict(name="d_coef", nbytes=coef.nbytes, align=16, role="in", row=4 * bs, rows_per_stream=ch * (N + 1)),
             dict(name="d_wc", nbytes=wc.nbytes, align=4, role="in", guard=wc.nbytes, row=4, rows_per_stream=N + 1),
             dict(name="d_pcm", nbytes=n * ch * N * bs * el, align=4 if pcm16 else 16, role="out", guard=ch * (N + 1) * bs * el, row=el * bs, rows_per_stream=ch * N),
             dict(name="d_live", nbytes=4 * n * N, align=4, role="out", guard=4 * n * (N + 1), row=4, rows_per_stream=N)]
    a = gb.build(torch.device("cuda", 0), specs)
    a.load("d_coef", coef); a.load("d_wc", wc)
    dec = _amd().BatchDecoder(n + 3, ch, bs, N + 2)                                           # (an object larger than the call)
    dec.synth_spectra_dev(n, N + 1, WARM, a.ptr("d_coef"), a.ptr("d_wc"), a.ptr("d_pcm"), a.ptr("d_live"), pcm16=pcm16)
    torch.cuda.synchronize()
    a.check()
    got = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(n, ch, N * bs)
    check_rows((got, a.fetch("d_live", np.int32).reshape(n, N)), (Y.to_pcm16(pcm) if pcm16 else pcm, live), bs, "guarded call")
    dec.close()


def test_corpus_binding_is_the_c_call():
    import torch
    import corpus
    amd = _amd()
    bs, ch = 2048, 2
    refs = Y.geom_streams((bs, ch))
    rows = Y.warm_rows(refs, total=8)
    coef, wc, pcm, live = Y.stack(refs, rows, N, 1)
    dec = amd.BatchDecoder(len(rows), ch, bs, N + 1)
    t_coef, t_wc = torch.from_numpy(coef).to("cuda:0"), torch.from_numpy(wc).to("cuda:0")
    for pcm16 in (False, True):
        p, l = corpus.synth_spectra(dec, t_coef, t_wc, warm=True, pcm16=pcm16)
        torch.cuda.synchronize()
        check_rows((p.cpu().numpy(), l.cpu().numpy()), (Y.to_pcm16(pcm) if pcm16 else pcm, live), bs, f"corpus.synth_spectra pcm16={pcm16}")
    p, l = corpus.synth_spectra(dec, t_coef, t_wc, warm=True, lr=True)
    torch.cuda.synchronize()
    assert same(p.cpu().numpy(), synth(dec, coef, wc, WARM | LR)[0])
    with pytest.raises(amd.UlcError):
        corpus.synth_spectra(dec, t_coef.double(), t_wc)
    with pytest.raises(amd.UlcError):
        corpus.synth_spectra(dec, t_coef, t_wc[:, :-1])
    with pytest.raises(amd.UlcError):
        corpus.synth_spectra(dec, t_coef[:, :1], t_wc)
    dec.close()
