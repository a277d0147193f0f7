"""The inputs of tests/test_gpu_writer_tiers.py, checked on the oracle alone: each has the property its GPU test is named for -
the boundary blocks keep exactly cap and cap + 1 coefficients, a single-cause block exceeds one capacity and stays at or
under 90 % of the others, the stereo batch holds every kind of hand-over, the decimated blocks fail in a unit behind the
first.  Without this a GPU test could pass on inputs that never leave the small tier.  Also the hooks' exports, binding and
the refusals that need no device, and the counts' own cross-checks (tests/writer_tiers_testlib.py).

The capacities here are writer_tiers_testlib.expected_plan's (small 512 / 128 / 1280, medium 1024 / 512 / 4096, the full tier
2048 / 1024 / 8256 at BlockSize 2048 and above); the GPU test takes them from ulcx_encoder_debug_writer_plan and pins them to
these values."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import writer_tiers_testlib as W

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_encoder_debug_writer_flags", "ulcx_encoder_debug_writer_plan")
SMALL, MEDIUM, FULL, plan_of = W.SMALL, W.MEDIUM, W.FULL, W.expected_plan


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    return C.CDLL(LIB)


def test_hooks_are_exported_and_bound(lib):
    import ulc_amd
    for n in NAMES:
        assert hasattr(lib, n) and n in ulc_amd.EXPORTS, n
    for m in ("writer_flags", "writer_plan"):
        assert hasattr(ulc_amd.BatchEncoder, m), m


def test_hooks_refuse_a_null_object_or_a_null_array(lib):
    lib.ulcx_last_error.restype = C.c_char_p
    live = C.c_void_p(16)                                  # (never dereferenced: the array is checked first)
    buf = (C.c_int32 * 16)()
    lib.ulcx_encoder_debug_writer_flags.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.ulcx_encoder_debug_writer_plan.argtypes = [C.c_void_p, C.c_void_p]
    for args, fn in (((None, 1, C.addressof(buf)), lib.ulcx_encoder_debug_writer_flags), ((live, 1, None), lib.ulcx_encoder_debug_writer_flags),
                     ((None, C.addressof(buf)), lib.ulcx_encoder_debug_writer_plan), ((live, None), lib.ulcx_encoder_debug_writer_plan)):
        assert fn(*args) == -1
        assert lib.ulcx_last_error().decode().startswith(fn.__name__ + ":")
    assert not any(buf)


def test_zone_restatement_on_hand_made_levels():
    z = W.zones_of
    assert z([]) == 0 and z([0.0]) == 0 and z([0.0, 0.0, 0.0]) == 0
    assert z([1.0]) == 1 and z([1.0, 4.0]) == 1 and z([1.0, 4.0001]) == 2           # max > 4 * min, not >=
    assert z([4.0, 1.0, 0.9]) == 2 and z([1.0, 2.0, 4.0, 8.0]) == 2
    assert z([5000.0, 1100.0]) == 2                         # the first minimum is capped at 1000: 5000 > 4 * 1000
    assert z([3000.0, 1100.0]) == 1                         # ... and the cap is a minimum, not a level: 3000 <= 4 * 1000
    assert z([1.0, 0.0]) == 1                               # a last zone of zero level is not counted
    assert z([1.0, 0.0, 1.0]) == 3
    assert z([-1.0, 2.0, -3.0]) == 1                        # levels are magnitudes


ALL_CASES = [lambda: W.boundary_case(2048, 512), lambda: W.boundary_case(2048, 1024), lambda: W.boundary_case(4096, 2048), W.full_never_fails_case,
             lambda: W.no_retry_case(512), lambda: W.no_retry_case(256), W.single_cause_case, lambda: W.gap_case(8192), lambda: W.gap_case(4096),
             W.stereo_case, lambda: W.decimated_case(2048), lambda: W.decimated_case(4096)] + [lambda c=c, m=m: W.rate_case(c, m) for c in (1, 2) for m in (1, 2)]


def test_counts_cross_checks_over_every_case():
    """Every unit of every case: the bytes carry no more quantizer-change codes than the restated rule has zones (a zone
    changes the quantizer at most once, and the opening one is no change); kept counts add up to nout; a unit that keeps
    nothing has no zone; the walk used every nybble of the block (block_units asserts it)."""
    units = least = 0
    for make in ALL_CASES:
        case = make()
        least += case.B * case.K * case.ch
        for s in range(case.B):
            for k, us in enumerate(case.units[s]):
                assert sum(u["nK"] for u in us) == min(int(case.refs[s]["nout"][k]), case.ch * case.bs), (case.name, s, k)
                for u in us:
                    assert u["changes"] <= max(u["nZ"] - 1, 0), (case.name, s, k, u)
                    assert u["nZ"] <= u["nK"] and u["nyb"] >= 2, (case.name, s, k, u)
                    units += 1
    assert units > least > 0                                # (more: every case has decimated blocks)


@pytest.mark.parametrize("bs,cap,tier,flags", [(2048, 512, SMALL, (0, 1)), (2048, 1024, MEDIUM, (1, 3)), (4096, 2048, FULL, (1, 3))])
def test_boundary_blocks_keep_exactly_cap_and_cap_plus_one(bs, cap, tier, flags):
    """... and nothing but K decides: at cap + 1 the zones and nybbles are within the tier, so the predicted flags differ
    between the two streams in K's bit alone.  (The medium tier is the exact path's retry.)"""
    case = W.boundary_case(bs, cap)
    plan = plan_of(bs)
    for s, want in enumerate((cap, cap + 1)):
        (u,) = case.units[s][W.BOUNDARY_BLOCK]
        print(case.name, "quality", -case.rates[s][0], u)
        assert u["nK"] == want == int(case.refs[s]["nout"][W.BOUNDARY_BLOCK])
        assert W.causes(u, tier) == ("K" if s else ""), u
        assert W.predict_flags([u], plan, 1, exact=(tier is MEDIUM)) == flags[s]


def test_full_tier_of_blocksize_1024_holds_everything():
    case = W.full_never_fails_case()
    plan = plan_of(1024)
    over = [us for s in range(case.B) for us in case.units[s] if any(W.causes(u, SMALL) for u in us)]
    assert len(over) >= 6 and any(u["nK"] == 1024 for us in over for u in us)         # (every coefficient of a block kept)
    assert not any(W.causes(u, plan["full"]) for us in over for u in us)


@pytest.mark.parametrize("bs", [512, 256])
def test_geometries_without_a_retry_tier_have_blocks_over_a_small_capacity(bs):
    """K cannot exceed 512 in a block of 512: these are Z inputs (more than 128 zones)."""
    case = W.no_retry_case(bs)
    plan = plan_of(bs)
    assert not plan["have_full"]
    flags, _ = case.predicted(plan)
    print(case.name, flags, [[W.causes(u, SMALL) for u in us] for us in case.units[0]])
    assert (flags == 2).sum() >= 3 and (flags == 0).sum() >= 1 and set(flags.ravel()) <= {0, 2}
    assert all("K" not in W.causes(u, SMALL) for us in case.units[0] for u in us)


def _alone(u, cause):
    """unit u is over the small capacity of `cause` and at or under 90 % of the other two (and G does not join in)"""
    i = "KZN".index(cause)
    v = (u["nK"], u["nZ"], u["nyb"])
    return v[i] > SMALL[i] and all(10 * v[j] <= 9 * SMALL[j] for j in range(3) if j != i) and u["gap"] <= W.GAP_NYBBLES


def test_single_cause_blocks_exceed_one_capacity_alone():
    case = W.single_cause_case()
    for s, cause in enumerate("ZN"):
        blocks = [us[0] for us in case.units[s] if len(us) == 1]
        alone = [u for u in blocks if _alone(u, cause)]
        print(cause, [(u["nK"], u["nZ"], u["nyb"]) for u in blocks])
        assert len(alone) >= 2, (cause, blocks)
        assert all(W.causes(u, MEDIUM) == "" for u in alone)                           # (under the exact path's retry: flags 1, not 3)
        assert all(W.causes(u, SMALL) in ("", cause) for u in blocks)


@pytest.mark.parametrize("bs", [8192, 4096])
def test_gap_blocks_have_one_gap_of_more_than_32_run_nybbles_and_nothing_else(bs):
    """G does not depend on the tier: such a block fails the small launch and the retry and is written by k_encode_units.
    BlockSize 4096 also holds a block whose longest gap is exactly 32 nybbles: it stays in the small tier."""
    case = W.gap_case(bs)
    units = [us[0] for s in range(case.B) for us in case.units[s] if len(us) == 1]
    print(bs, [(u["nK"], u["nZ"], u["nyb"], u["gap"]) for u in units])
    g = [u for u in units if u["gap"] > W.GAP_NYBBLES]
    assert len(g) >= 4 and all(W.causes(u, SMALL) == "G" == W.causes(u, FULL) for u in g)
    assert all(10 * u["nK"] <= 9 * SMALL[0] and 10 * u["nZ"] <= 9 * SMALL[1] and 10 * u["nyb"] <= 9 * SMALL[2] for u in g)
    if bs == 4096:
        assert any(u["gap"] == W.GAP_NYBBLES for u in units)
    flags, _ = case.predicted(plan_of(bs))
    assert set(flags.ravel()) == {0, 3}


def test_stereo_batch_holds_every_kind_of_hand_over():
    case = W.stereo_case()
    kinds = {}
    for s in range(case.B):
        for k, us in enumerate(case.units[s]):
            if W.whole(us, 2) and int(case.refs[s]["nout"][k]) > 0:
                kinds.setdefault(W.stereo_kind(us, SMALL), []).append((s, k))
    print(kinds)
    assert set(kinds) == set(W.STEREO_KINDS) and all(len(v) >= 3 for v in kinds.values())
    # the healthy channel of a one-sided block is far below every capacity: the hand-over is the other channel's alone
    for kind, c_ok in (("channel 0 only", 1), ("channel 1 only", 0)):
        for s, k in kinds[kind]:
            u = case.units[s][k][c_ok]
            assert 2 * u["nK"] <= SMALL[0] and 2 * u["nZ"] <= SMALL[1] and 2 * u["nyb"] <= SMALL[2], (kind, s, k, u)
    flags, _ = case.predicted(plan_of(2048))
    for kind, where in kinds.items():
        assert all(flags[s, k] == (4 if kind == "neither" else 1) for s, k in where), kind


@pytest.mark.parametrize("bs", [2048, 4096])
def test_decimated_case_fails_in_a_unit_behind_the_first_only(bs):
    case = W.decimated_case(bs)
    found = []
    for k, us in enumerate(case.units[0]):
        bad = [(u["ch"], u["j"]) for u in us if W.causes(u, SMALL)]
        if len(us) > 2 and bad and all(j >= 1 for _, j in bad):
            found.append((k, bad))
            assert not any(W.causes(u, FULL) for u in us)
    print(case.name, found)
    assert found and any(len(bad) == 1 for _, bad in found)


@pytest.mark.parametrize("ch,mode", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_rate_search_settings_end_above_the_medium_tier(ch, mode):
    case = W.rate_case(ch, mode)
    n = sum(1 for s in range(case.B) for us in case.units[s] if any("K" in W.causes(u, MEDIUM) for u in us) and not any(W.causes(u, FULL) for u in us))
    assert n >= 6, n


def test_ladder_rungs_differ_in_every_tier_they_reach():
    plan = plan_of(2048)
    dense, _ = W.ladder_case(W.LADDER_DENSE).predicted(plan)
    sparse, _ = W.ladder_case(W.LADDER_SPARSE).predicted(plan)
    print(dense, sparse, sep="\n")
    assert (dense != sparse).sum() >= 6 and (dense == 1).sum() >= 6 and (sparse == 4).sum() >= 6
