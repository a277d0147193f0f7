"""The wave writer's capacity hand-overs, cause by cause (k_encode_wave -> k_encode_wave retry -> k_encode_units; the
stereo direct-packing protocol on top).  Every case encodes through BatchEncoder and compares sizes, WindowCtrl,
BlockComplexity and bytes with the oracle block by block; then it asserts, for every block, that the tier the block ended
in (ulcx_encoder_debug_writer_flags) is the one predicted from the oracle's counts alone and the reported capacities
(tests/writer_tiers_testlib.py), and that each kind the case is named for occurs - a census, as `assert nfb > 256` is for
the exact path.  A hand-over that is never taken, always taken, or reaches the serial kernel too early leaves every byte
right; these tests see it.  tests/test_writer_tiers_capi.py checks on the CPU that the inputs have the properties named here.

Where the prediction departs from the plain reading "a block over a small capacity ends with flags 1":
  * cause G (the run codes of one gap exceed 32 nybbles) does not depend on the tier, so a G block fails the retry too and
    is written by the serial kernel: flags 3 (2 where there is no retry).
  * the exact path's launches pack directly as well while its blocks fit its grid of min(blocks, 128) workgroups in one trip;
    bit 2 is withheld only beyond that (test_stereo_exact_path_at_scale_stands_back_from_direct_packing).
  * a block that keeps nothing never reaches the exact path, whatever ulcx_encoder_debug_force_exact says."""
import os
import numpy as np
import pytest

from gpu_testlib import amd as _amd
import writer_tiers_testlib as W

pytestmark = pytest.mark.gpu


def _encoder(case, K, env=None):
    """BatchEncoder for the case's geometry with its reported plan, pinned to what enc_plan gives for the BlockSize"""
    amd = _amd()
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        enc = amd.BatchEncoder(case.B, case.ch, case.bs, case.rate, K)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    plan = enc.writer_plan()
    assert plan == W.expected_plan(case.bs), (case.bs, plan)
    return enc, plan


def _compare_bytes(res, refs, k0, K, what):
    out, bits, wc, cplx = res
    for s, ref in enumerate(refs):
        for k in range(K):
            kk, tag = k0 + k, f"{what}: stream {s} block {k0 + k}"
            assert wc[s, k] == ref["wc"][kk], f"{tag}: WindowCtrl {wc[s, k]:#x} != {ref['wc'][kk]:#x}"
            assert cplx[s, k].tobytes() == ref["cplx"][kk].tobytes(), f"{tag}: BlockComplexity"
            assert bits[s, k] == ref["bits"][kk], f"{tag}: size {bits[s, k]} != {ref['bits'][kk]}"
            nb = bits[s, k] // 8
            assert np.array_equal(out[s, k, :nb], ref["out"][kk, :nb]), f"{tag}: stream bytes differ"


def _run(case, census, every=0, env=None, calls=1):
    """Encode the case in `calls` calls; bytes, exact-path count and flags of every call against the oracle and the prediction.
    census: the flag values that must occur among the predicted ones of the whole case.  -> (flags, predicted) [B][K]."""
    amd = _amd()
    K = case.K // calls
    enc, plan = _encoder(case, K, env)
    direct = (env or {}).get("ULCX_DIRECT_PACK", "1") != "0"
    enc.force_exact(every)
    got, want = [], []
    for c in range(calls):
        pcm = case.pcm[:, c * K * case.bs:(c + 1) * K * case.bs]
        res = enc.encode_rates(pcm, case.rates) if case.rates is not None else enc.encode(pcm, case.mode, case.p0, case.p1)
        _compare_bytes(res, case.refs, c * K, K, f"{case.name} every={every} {env or ''}")
        flags, nfb = enc.writer_flags(), enc.last_fallbacks()
        pred, exact = case.predicted(plan, every, direct, c * K, K)
        print(f"{case.name} every={every} {env or ''} call {c}: exact path {nfb} (predicted {int(exact.sum())})\nflags\n{flags}\npredicted\n{pred}")
        assert nfb == int(exact.sum()), f"{case.name}: {nfb} blocks on the exact path, {int(exact.sum())} predicted"
        got.append(flags); want.append(pred)
    enc.close()
    got, want = np.concatenate(got, axis=1), np.concatenate(want, axis=1)
    assert set(census) <= set(int(v) for v in want.ravel()), f"{case.name}: the input does not reach {set(census) - set(want.ravel())}"
    assert np.array_equal(got, want), f"{case.name}: tiers differ from the prediction at (stream, block) {np.argwhere(got != want).tolist()}"
    return got, want


def test_hooks_refuse_without_a_last_encode_call_and_report_the_plan():
    amd = _amd()
    case = W.no_retry_case(256)
    enc, plan = _encoder(case, case.K)
    assert not plan["have_full"] and not plan["have_mid"]
    with pytest.raises(amd.UlcError, match="ulcx_encoder_debug_writer_flags"):
        enc.writer_flags(case.K)                             # no call yet
    enc.encode(case.pcm, amd.MODE_VBR, 100.0)
    assert enc.writer_flags().shape == (1, case.K)
    with pytest.raises(amd.UlcError, match="ulcx_encoder_debug_writer_flags"):
        enc.writer_flags(case.K - 1)                         # not the last call's nBlocks
    enc.analyse(case.pcm)
    with pytest.raises(amd.UlcError, match="ulcx_encoder_debug_writer_flags"):
        enc.writer_flags(case.K)                             # an analysis call ran no writer
    enc.close()


def test_boundary_of_the_small_tier_512_and_513_kept():
    """2048 x 1: the block with 512 kept coefficients stays in the small launch (flags 0), the one with 513 leaves it (1) - one
    stream per value under a per-stream VBR table, then the plain scalar call once per value (the path callers use)."""
    amd = _amd()
    case = W.boundary_case(2048, 512)
    got, _ = _run(case, {0, 1})
    assert got[:, W.BOUNDARY_BLOCK].tolist() == [0, 1]
    for s in range(2):
        one = W.Case(f"{case.name}, scalar call {s}", case.bs, 1, case.pcm, mode=0, p0=-float(case.rates[s][0]))
        got, _ = _run(one, {s})
        assert got[:, W.BOUNDARY_BLOCK].tolist() == [s, s]


def test_boundary_of_the_medium_tier_on_the_exact_path_1024_and_1025_kept():
    """2048 x 1, every block on the exact path, whose retry runs with the medium capacities: 1024 kept -> 1, 1025 -> 3 (the
    serial kernel, from the exact path).  _run checks last_fallbacks() == the blocks that keep anything."""
    case = W.boundary_case(2048, 1024)
    got, _ = _run(case, {1, 3}, every=1)
    assert got[:, W.BOUNDARY_BLOCK].tolist() == [1, 3]
    got, _ = _run(case, {1})                                 # the main path retries with the full capacities: both 1
    assert got[:, W.BOUNDARY_BLOCK].tolist() == [1, 1]


def test_boundary_of_the_halved_full_tier_2048_and_2049_kept():
    """4096 x 1: the full tier is halved to 2048 / 1024 / 8256, so a unit of 2049 kept coefficients ends in the serial kernel
    from the main path's final pass."""
    got, _ = _run(W.boundary_case(4096, 2048), {1, 3})
    assert got[:, W.BOUNDARY_BLOCK].tolist() == [1, 3]


@pytest.mark.parametrize("every", [0, 1])
def test_full_tier_of_blocksize_1024_never_fails(every):
    """1024 x 1, white noise at quality 100: full is the whole unit (and there is no medium tier, on either path)"""
    got, _ = _run(W.full_never_fails_case(), {1}, every=every)
    assert not (got & 2).any() and (got == 1).sum() >= 6


@pytest.mark.parametrize("bs", [512, 256])
def test_geometries_without_a_retry_tier_go_straight_to_the_serial_kernel(bs):
    """One launch of the wave writer: a block over a small capacity (Z: more than 128 zones) has flags 2, never bit 0"""
    got, _ = _run(W.no_retry_case(bs), {0, 2})
    assert not (got & 1).any()


@pytest.mark.parametrize("every", [0, 1])
def test_single_causes_z_alone_and_n_alone(every):
    """2048 x 1: more than 128 zones with K and N under 90 % of their capacities; more than 1280 nybbles likewise.  Flags 1 on
    the main path, and 1 on the exact path as well: both are within the medium tier."""
    case = W.single_cause_case()
    got, _ = _run(case, {0, 1}, every=every)
    assert (got[0] == 1).sum() >= 2 and (got[1] == 1).sum() >= 2


@pytest.mark.parametrize("bs,every", [(8192, 0), (8192, 1), (4096, 0), (4096, 1)])
def test_single_cause_g_fails_every_wave_tier(bs, every):
    """One gap of more than 32 run-code nybbles in a block far below every capacity: no wave tier holds it, flags 3.  4096:
    a block whose longest gap is exactly 32 nybbles stays in the small launch."""
    _run(W.gap_case(bs), {0, 3}, every=every)


def _kinds(case):
    return np.array([[W.stereo_kind(us, W.SMALL) if W.whole(us, 2) else "decimated" for us in case.units[s]] for s in range(case.B)])


def test_stereo_direct_packing_hand_overs():
    """2048 x 2, the four kinds of un-decimated block: bit 2 exactly on "neither"; a failing channel 0 beside a healthy
    channel 1 (its fail mark passed through the LDS word) and the reverse (channel 0 has already written its bytes into the
    slot) come out byte-equal through the retry and k_pack, flags 1."""
    case = W.stereo_case()
    got, _ = _run(case, {1, 4})
    kinds = _kinds(case)
    assert set(W.STEREO_KINDS) <= set(kinds.ravel())
    assert np.array_equal(got == 4, kinds == "neither")
    for kind in W.STEREO_KINDS[1:]:
        assert (got[kinds == kind] == 1).all(), kind


def test_stereo_without_direct_packing_same_bytes_no_bit_2():
    got, want = _run(W.stereo_case(), {0, 1}, env={"ULCX_DIRECT_PACK": "0"})
    assert not (got & 4).any()


def test_stereo_exact_path_within_one_trip_packs_directly():
    """The same batch on the exact path (24 blocks, 20 of them keep something): its launch covers them in one trip"""
    got, _ = _run(W.stereo_case(), {1, 4}, every=1)
    assert (got == 4).sum() >= 4


def test_stereo_exact_path_at_scale_stands_back_from_direct_packing():
    """44 streams (the four, eleven times) x 6 blocks x 2 calls, every block on the exact path.  Call 0: 220 blocks keep
    something, 440 waves of work on a grid of 128 x 4 - one trip, bit 2 on "neither".  Call 1: 264 blocks, 528 waves - a
    second trip for some, so no block of that path is packed directly: no bit 2.  (One group of rank slots: the call's
    blocks fit a quarter of the device's free memory many times over.)"""
    case = W.stereo_case(tile=11, n_blocks=12)
    got, _ = _run(case, {0, 1, 4}, every=1, calls=2)
    assert (got[:, 1:6] & 4).any() and not (got[:, 6:] & 4).any()


@pytest.mark.parametrize("bs", [2048, 4096])
def test_decimated_block_whose_only_failing_unit_is_not_the_first(bs):
    """A burst late in a block of dense noise: the block decimates, and one unit with j >= 1 is the only one over a small
    capacity (its other units have written unitNyb / unitBuf already): flags 1 for the whole block, bytes equal."""
    case = W.decimated_case(bs)
    got, _ = _run(case, {1})
    hit = [k for k, us in enumerate(case.units[0]) if len(us) > 2 and [u["j"] for u in us if W.causes(u, W.SMALL)] not in ([], [0]) and
           all(u["j"] >= 1 for u in us if W.causes(u, W.SMALL))]
    assert hit and all(got[0, k] == 1 for k in hit)


@pytest.mark.parametrize("ch,mode", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_rate_search_ends_above_the_medium_tier(ch, mode):
    """2048 x ch under CBR and ABR at rates whose final nout puts a unit above 1024 kept coefficients: the probes' retries run
    on the medium tier and overflow it, the final pass retries with the full one (flags 1).  Two calls.  The hook shows the
    final pass only (every pass clears the flags): the probes' own tiers are not observable through it - sizes and bytes
    equal to the oracle's are what says the probes measured right."""
    got, _ = _run(W.rate_case(ch, mode), {1}, calls=2)
    assert (got == 1).sum() >= 6


@pytest.mark.parametrize("order", [(W.LADDER_DENSE, W.LADDER_SPARSE), (W.LADDER_SPARSE, W.LADDER_DENSE)])
def test_ladder_flags_are_the_last_rungs(order):
    """2048 x 2, two VBR rungs in both orders: a rung armed by k_rung_arm starts from cleared flags, so after the call the
    flags are the last rung's alone (dense last: 1 where a channel is over; sparse last: nothing left of the dense rung)."""
    amd = _amd()
    rungs = [W.ladder_case(q) for q in order]
    case = rungs[-1]
    enc, plan = _encoder(case, case.K)
    out, bits, wc, cplx = enc.encode_ladder(case.pcm, [(amd.MODE_VBR, q) for q in order])
    for r, rung in enumerate(rungs):
        _compare_bytes((out[r], bits[r], wc, cplx), rung.refs, 0, case.K, f"ladder {order} rung {r}")
    flags, nfb = enc.writer_flags(), enc.last_fallbacks()
    enc.close()
    want = [rung.predicted(plan) for rung in rungs]
    print(f"ladder {order}: exact path {nfb}\nflags\n{flags}\nfirst rung predicted\n{want[0][0]}\nlast rung predicted\n{want[1][0]}")
    assert nfb == sum(int(e.sum()) for _, e in want)
    assert (want[0][0] != want[1][0]).sum() >= 6
    assert np.array_equal(flags, want[1][0]), np.argwhere(flags != want[1][0]).tolist()
