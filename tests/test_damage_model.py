"""The premises of tests/test_gpu_damaged_crops.py, checked on the CPU with the oracle alone: the range-local model
(damage_testlib.local_model) equals the oracle's sequential decode on clean payloads, and the damaged copies the GPU tests use
are what they are named - a kill ends the row at its block, a value damage changes samples and no size, and a damage is local
to the rows whose blocks, the block in front included, contain it."""
import numpy as np
import pytest

import damage_testlib as D
from seek_testlib import oracle_pcm, expected_range, switched_starts

N = 4


@pytest.mark.parametrize("geom", D.GEOMS)
def test_model_equals_the_slice_of_the_sequential_decode_on_clean_payloads(geom):
    st = D.stream_of(geom)
    ref, rbits = oracle_pcm(st.blocks, st.ch, st.bs)
    sw = switched_starts(st.wc)
    assert len(sw) >= 2, f"{st.name}: {len(sw)} starts behind a window-switched block"
    starts = [0, 1, 5] + sw[:4] + [st.K - 2, st.K - 1, st.K]          # (the last three run past the end: live < N)
    for first in starts:
        pcm, bits, live = st.model(st.payload, first, N)
        want, wb = expected_range(ref, rbits, first, N)
        assert live == max(0, min(N, st.K - first)), (first, live)
        assert np.array_equal(bits, wb), f"{st.name} from block {first}: bits {bits} vs {wb}"
        assert D.same_bytes(pcm, want), f"{st.name} from block {first}: the model differs from the sequential decode"
    assert st.model(st.payload, -1, N)[2] == 0 and st.model(st.payload, st.K + 1, N)[2] == 0
    for count in (-1, 0, 2, N, N + 3):                      # d_count: the leading blocks, clamped to [0, N]
        pcm, bits = D.expected_crop_row(st.payload, st.offs, st.seeds, st.ch, st.bs, 5, N, count)
        m = max(0, min(N, count))
        assert np.array_equal(bits[:m], rbits[5:5 + m]) and D.same_bytes(pcm[:m], ref[5:5 + m]) and not bits[m:].any() and not pcm[m:].any(), count
    # the sample form: a crop that straddles blocks, one with a length, one running past the end
    stream = ref.reshape(st.K * st.bs, st.ch).T
    for start, ns, ln in ((sw[0] * st.bs - 3, 2 * st.bs + 3, None), (5 * st.bs + 1, 2 * st.bs + 3, st.bs), ((st.K - 1) * st.bs + 7, st.bs + 1, None)):
        out, bits = D.expected_sample_row(st.payload, st.offs, st.seeds, st.ch, st.bs, start, ns, ln)
        n = ns if ln is None else ln
        end = min(start + n, st.K * st.bs)
        want = np.zeros((st.ch, ns), np.float32)
        want[:, :end - start] = stream[:, start:end]
        assert D.same_bytes(out, want), (st.name, start, ns, ln)
        touched = [b for b in range(start // st.bs, (start + n - 1) // st.bs + 1) if b < st.K]
        assert np.array_equal(bits[:len(touched)], rbits[touched]) and (bits[len(touched):] == 0).all(), (st.name, start, bits)


@pytest.mark.parametrize("geom", D.GEOMS)
def test_damages_are_what_they_are_named(geom):
    st = D.stream_of(geom)
    cor = D.geometry_corpus(geom)
    pos = D.positions_of(geom)
    assert len(pos) == 3 and int(st.wc[pos[2]]) != 0x10, f"{st.name}: no window-switched block among the damaged positions {pos}"
    kinds = {j: [kd for kd, p, _ in cor.files if p == j] for j in pos}
    print(f"{st.name}: " + "; ".join(f"block {j}: " + ", ".join(f"{kd} (seed {sd})" for kd, p, sd in cor.files if p == j) for j in pos))
    for j in pos:
        assert "kill" in kinds[j] and "value" in kinds[j], (j, kinds[j])
        if "resize" not in kinds[j]:
            print(f"{st.name}: no seed below {D.MAX_SEED} resizes block {j} and leaves the row alive")
    assert any("draws" in kinds[j] for j in pos), f"{st.name}: no damage displaces the generator"
    _check_classes(cor)


def _check_classes(cor, n=N):
    """Every damaged file of the corpus, every place of its damaged block in a row of n blocks."""
    st = cor.st
    clean = lambda first, m=n: st.model(st.payload, first, m)
    for f, (kind, j, sd) in enumerate(cor.files):
        if kind == "clean":
            continue
        what = f"{st.name}: {kind} of block {j} (seed {sd})"
        for first, place in D.rows_around(j):
            if first < 0 or first > st.K:
                continue
            pcm, bits, live = cor.model(f, first, n)
            cp, cb, cl = clean(first)
            if place in ("behind the row", "in front of the warm block"):
                assert live == cl and np.array_equal(bits, cb) and D.same_bytes(pcm, cp), f"{what}: the row from {first} ({place}) is not the clean one"
                continue
            at = j - first                                  # the damaged block's place in the row; -1: the block in front
            if kind == "kill":
                assert live == max(0, at), f"{what}: the row from {first} ({place}) lives {live} blocks"
                assert (bits[:live] > 0).all() and (bits[live:] == 0).all() and not pcm[live:].any(), what
                assert D.same_bytes(pcm[:live], cp[:live]) and np.array_equal(bits[:live], cb[:live]), f"{what}: blocks in front of the dead one changed"
            else:
                assert live == cl == min(n, st.K - first), f"{what}: the row from {first} ({place}) lives {live} of {cl} blocks"
                assert (bits[:live] > 0).all(), what
                assert (kind == "resize" and at >= 0) == (not np.array_equal(bits, cb)), f"{what}: sizes {bits} vs the clean {cb}"
                if at >= 0:
                    assert np.array_equal(np.delete(bits, at), np.delete(cb, at)), f"{what}: another block's size changed"
                    assert D.same_bytes(pcm[:at], cp[:at]), f"{what}: a block in front of the damage changed"
                    assert kind == "resize" or not D.same_bytes(pcm[at], cp[at]), f"{what}: the damaged block's samples did not change"
                    assert at + 1 >= live or not D.same_bytes(pcm[at:], cp[at:]), f"{what}: row from {first}: no sample changed"
                changed = [k for k in range(max(at + 1, 0), live) if not D.same_bytes(pcm[k], cp[k])]
                if at + 1 < live and kind != "resize":      # (a resize may change a late sub-block alone: its samples leave with the next block)
                    assert changed and changed[0] == max(at + 1, 0), f"{what}: row from {first}: no later block changed ({changed})"
                if kind == "draws" and at + 2 < live:
                    assert at + 2 in changed, f"{what}: row from {first}: block {j + 2} is the clean one - the generator did not move"
            if live > 0:
                assert pcm.any(), f"{what}: the row from {first} is all zeros"
            else:
                assert kind == "kill" and at <= 0


def test_the_sweep_corpora_kill_and_damage_every_block():
    """The 31 files of the cut-launch tests: file j is killed (or its values damaged) at block j; rows of 30 and 36 blocks from
    block 1 end there (or change from there on) and nowhere else."""
    st = D.stream_of(D.SWEEP_GEOM)
    assert st.K == 40
    cp, cb, cl = st.model(st.payload, 1, 36)
    assert cl == 36 and (cb > 0).all()
    for kind in ("kill", "value"):
        cor = D.sweep_corpus(kind)
        assert cor.F == D.SWEEP_FILES and [j for _, j, _ in cor.files] == list(range(D.SWEEP_FILES))
        # (block 0 of this stream is three bytes of silence: every nybble of it either kills it or lies behind its last bit)
        assert [kd for kd, _, _ in cor.files] == [kind] * D.SWEEP_FILES if kind == "kill" else [kd for kd, _, _ in cor.files[1:]] == [kind] * (D.SWEEP_FILES - 1)
        displaced = 0
        for j in range(cor.F):
            pcm, bits, live = cor.model(j, 1, 36)
            if kind == "kill":
                assert live == max(0, j - 1) and not pcm[live:].any() and (bits[live:] == 0).all(), (j, live)
                assert D.same_bytes(pcm[:live], cp[:live]) and np.array_equal(bits[:live], cb[:live]), j
            elif cor.files[j][0] == "intact":
                assert j == 0 and live == 36 and np.array_equal(bits, cb) and D.same_bytes(pcm, cp)
            else:
                at = j - 1
                assert live == 36 and np.array_equal(bits, cb), (j, live)
                assert D.same_bytes(pcm[:max(at, 0)], cp[:max(at, 0)]) and not D.same_bytes(pcm[at + 1], cp[at + 1]), j
                assert not D.same_bytes(pcm[at], cp[at]), j
                displaced += not D.same_bytes(pcm[-1], cp[-1])
        if kind == "value":
            print(f"{displaced} of {cor.F} value damages displace the generator to the row's end")
            assert displaced >= cor.F // 2, displaced        # (the prefix sums of the draws matter to most rows)


def test_kill_falls_back_to_the_fill():
    """kill_block's fallback, the 0x11 fill of tests/test_gpu_parity.py, ends the row under the model too."""
    for geom in ((2048, 2), (512, 1), (1024, 6)):
        st = D.stream_of(geom)
        pay = D.fill_block(st.payload, st.offs, 7)
        assert pay.shape == st.payload.shape
        assert st.model(pay, 7, 2)[2] == 0 and st.model(pay, 5, N)[2] == 2 and st.model(pay, 8, 2)[2] == 0 and st.model(pay, 9, 2)[2] == 2


def test_damage_block_is_one_nybble_inside_the_block():
    st = D.stream_of((2048, 2))
    hit_first = hit_last = False
    for k in (0, 7, st.K - 1):
        for seed in range(200):
            pay = D.damage_block(st.payload, st.offs, k, seed)
            diff = np.flatnonzero(pay != st.payload)
            assert len(diff) == 1 and st.offs[k] <= diff[0] < st.offs[k + 1], (k, seed, diff)
            x = int(pay[diff[0]]) ^ int(st.payload[diff[0]])
            assert (x & 0x0F) == 0 or (x & 0xF0) == 0, (k, seed)
            hit_first |= diff[0] < st.offs[k] + (st.offs[k + 1] - st.offs[k]) // 8
            hit_last |= diff[0] >= st.offs[k + 1] - (st.offs[k + 1] - st.offs[k]) // 8
            assert np.array_equal(pay, D.damage_block(st.payload, st.offs, k, seed))
    assert hit_first and hit_last, "the damages do not reach both ends of the extent"
