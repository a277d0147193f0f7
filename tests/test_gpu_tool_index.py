"""The front-end's block index files on the GPU: `ulcx-tool encode -index` writes a `.ulx` sidecar beside every `.ulc`
(include/ulc_amd.h section 3) whose entries are ulcx_index_packed_host's of the file's payload, and `decode -blocks:` writes
the same bytes with the sidecar, without it, and with one it has to refuse."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ulc_testlib import synth_pcm, run_tool, write_wav16

pytestmark = pytest.mark.gpu
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")
RATE, BS, CH = 44100, 2048, 2
FRAMES = (9 * BS + 100, 5 * BS)                             # two short files of different length: 12 and 7 blocks


@pytest.fixture(scope="module")
def encoded(tmp_path_factory):
    """a.wav, b.wav encoded once with -index as a two-rung ladder and once plainly -> (dir of the ladder, dir of the plain run)"""
    d = tmp_path_factory.mktemp("ulx")
    wavs = []
    for i, n in enumerate(FRAMES):
        p = d / f"{'ab'[i]}.wav"
        write_wav16(p, np.rint(synth_pcm(30 + i, n, CH, RATE, transient=True, seed=4) * 32768.0), RATE)
        wavs.append(str(p))
    lad, one = d / "ladder", d / "one"
    lad.mkdir(); one.mkdir()
    r = run_tool([TOOL, "encode", str(lad), "-50/64", "-index"] + wavs, check=False)
    assert r.returncode == 0, r.stderr.decode()
    r = run_tool([TOOL, "encode", str(one), "-50", "-index"] + wavs, check=False)
    assert r.returncode == 0, r.stderr.decode()
    return lad, one


def _payload(path):
    import ulc_amd
    data = open(path, "rb").read()
    h = ulc_amd.FileHeader.from_buffer_copy(data[:24])
    return h, np.frombuffer(data[h.StreamOffs:], np.uint8)


def test_encode_index_writes_the_packed_index_of_every_file(encoded):
    import ulc_amd
    lad, one = encoded
    names = sorted(os.listdir(lad))
    assert names == ["a.r0.ulc", "a.r0.ulx", "a.r1.ulc", "a.r1.ulx", "b.r0.ulc", "b.r0.ulx", "b.r1.ulc", "b.r1.ulx"], names
    assert sorted(os.listdir(one)) == ["a.ulc", "a.ulx", "b.ulc", "b.ulx"]
    files = [lad / n for n in names if n.endswith(".ulc")] + [one / "a.ulc", one / "b.ulc"]
    dec = ulc_amd.BatchDecoder(1, CH, BS, 2)
    for f in files:
        h, pay = _payload(f)
        assert h.nBlocks == (FRAMES[0 if f.name[0] == "a" else 1] + BS - 1) // BS + 2
        xh, ent = ulc_amd.ulx_parse(open(str(f)[:-1] + "x", "rb").read())
        assert (xh.BlockSize, xh.nChan, xh.nBlocks, xh.PayloadBytes) == (BS, CH, h.nBlocks, pay.size), f.name
        assert os.path.getsize(str(f)[:-1] + "x") == 16 + 8 * (h.nBlocks + 1)
        index, count = dec.index_packed(pay[None, :], np.array([pay.size], np.int32), h.nBlocks)
        assert count[0] == h.nBlocks and index["ByteOffs"][0, h.nBlocks] == pay.size, f.name
        assert np.array_equal(ent, index[0]), f"{f.name}: the sidecar differs from ulcx_index_packed_host of the payload"
        assert ulc_amd.index_check(ent, h.nBlocks, pay.size)
    dec.close()
    # the sidecar changes nothing in the container: the plain run's files are rung 0's
    for n in "ab":
        assert open(one / f"{n}.ulc", "rb").read() == open(lad / f"{n}.r0.ulc", "rb").read()


def test_decode_blocks_writes_the_same_bytes_with_without_and_with_a_refused_sidecar(encoded, tmp_path):
    _, one = encoded
    NOTICE = b"indexing the payloads"
    outs = {}
    for tag in ("with", "without", "altered", "checked"):
        src = tmp_path / f"in_{tag}"
        src.mkdir()
        for n in "ab":
            open(src / f"{n}.ulc", "wb").write(open(one / f"{n}.ulc", "rb").read())
            x = bytearray(open(one / f"{n}.ulx", "rb").read())
            if tag == "altered" and n == "b":
                x[8] ^= 1                                   # the header's block count: no longer the container's
            if tag == "checked" and n == "a":
                x[16 + 8 * 3:16 + 8 * 3 + 4] = x[16 + 8 * 2:16 + 8 * 2 + 4]      # entry 3 starts where entry 2 does: the header agrees, ulcx_index_check does not
            if tag != "without":
                open(src / f"{n}.ulx", "wb").write(bytes(x))
        dst = tmp_path / f"out_{tag}"
        dst.mkdir()
        r = run_tool([TOOL, "decode", str(dst), "-format:FLOAT32", "-blocks:3,4", str(src / "a.ulc"), str(src / "b.ulc")], check=False)
        assert r.returncode == 0, r.stderr.decode()
        outs[tag] = {n: open(dst / f"{n}.wav", "rb").read() for n in "ab"}
        assert (NOTICE in r.stderr) == (tag != "with"), (tag, r.stderr.decode())
        if tag == "altered":
            assert b"b.ulc" in r.stderr and b"header mismatch" in r.stderr, r.stderr.decode()
        if tag == "checked":
            assert b"a.ulc" in r.stderr and b"ulcx_index_check" in r.stderr, r.stderr.decode()
    full = tmp_path / "full"
    full.mkdir()
    r = run_tool([TOOL, "decode", str(full), "-format:FLOAT32", str(one / "a.ulc"), str(one / "b.ulc")], check=False)
    assert r.returncode == 0, r.stderr.decode()
    bpf = CH * 4 * BS
    for n in "ab":
        want = open(full / f"{n}.wav", "rb").read()[44 + 3 * bpf:44 + 7 * bpf]
        assert len(want) == 4 * bpf
        for tag, o in outs.items():
            assert len(o[n]) == 44 + 4 * bpf and o[n][44:] == want, f"{n}.wav, sidecar {tag}: differs from the full decode's bytes"
