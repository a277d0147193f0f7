"""Per-stream rate settings on the oracle side: one orc_encoder per stream, driven block by block through
orc_encode_block_{vbr,cbr,abr} (oracle/ulc_oracle.h:99-106), so that a stream's setting may change from one block
to the next.  A setting is (RateKbps, AvgComplexity) in the reference tool's convention (ulcEncodeTool.c:157-159)."""
import ctypes as C
import numpy as np
from ulc_testlib import oracle, f32p, u8p


class OrcTransient(C.Structure):
    _fields_ = [("Sum", C.c_float), ("SumW", C.c_float)]


class OrcEncoder(C.Structure):
    """oracle/ulc_oracle.h:40-57"""
    _fields_ = [("RateHz", C.c_int), ("nChan", C.c_int), ("BlockSize", C.c_int), ("WindowCtrl", C.c_int), ("NextWindowCtrl", C.c_int),
                ("BlockComplexity", C.c_float), ("TransientFilter", C.c_float * 3),
                ("SampleBuffer", C.c_void_p), ("TransformBuffer", C.c_void_p), ("TransformNoise", C.c_void_p), ("TransformFwdLap", C.c_void_p),
                ("TransformTemp", C.c_void_p), ("TransformIndex", C.POINTER(C.c_int32)), ("Keys", C.c_void_p), ("Masking", C.c_void_p),
                ("MDSTdbg", C.c_void_p), ("TransientBuffer", OrcTransient * 16), ("nNzCoef", C.c_int), ("lastNOutCoef", C.c_int)]


def _lib():
    lib = oracle()
    if not getattr(lib, "_rates_bound", False):
        lib.orc_encoder_init.argtypes = [C.POINTER(OrcEncoder)]
        lib.orc_encoder_destroy.argtypes = [C.POINTER(OrcEncoder)]
        lib.orc_encode_block_vbr.argtypes = [C.POINTER(OrcEncoder), u8p, f32p, C.c_float]
        lib.orc_encode_block_cbr.argtypes = [C.POINTER(OrcEncoder), u8p, f32p, C.c_float]
        lib.orc_encode_block_abr.argtypes = [C.POINTER(OrcEncoder), u8p, f32p, C.c_float, C.c_float]
        lib._rates_bound = True
    return lib


def mode_of(setting):
    """(mode, p0, p1) of the scalar API for a per-stream entry: 0 VBR(Quality), 1 CBR(kbps), 2 ABR(kbps, complexity)."""
    r, a = np.float32(setting[0]), np.float32(setting[1])
    if r < 0:
        return 0, float(-r), 0.0
    if a > 0:
        return 2, float(r), float(a)
    return 1, float(r), 0.0


class OracleStream:
    """One stream of the oracle encoder, one block per call."""

    def __init__(self, n_chan, block_size, rate_hz):
        self.lib = _lib()
        self.st = OrcEncoder()
        self.st.RateHz, self.st.nChan, self.st.BlockSize = rate_hz, n_chan, block_size
        assert self.lib.orc_encoder_init(C.byref(self.st)) == 1
        self.cb = n_chan * block_size
        self.tmp = np.zeros(4 * self.cb + 64, np.uint8)

    def close(self):
        if self.st.SampleBuffer:
            self.lib.orc_encoder_destroy(C.byref(self.st))
            self.st.SampleBuffer = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def block(self, pcm_block, setting):
        """pcm_block [BlockSize][nChan] f32 -> dict(bytes, bits, wc, cplx, nout, keep[nChan*BlockSize] uint8)."""
        src = np.ascontiguousarray(pcm_block, dtype=np.float32).reshape(-1)
        mode, p0, p1 = mode_of(setting)
        dst, sp = self.tmp.ctypes.data_as(u8p), src.ctypes.data_as(f32p)
        if mode == 0:
            bits = self.lib.orc_encode_block_vbr(C.byref(self.st), dst, sp, p0)
        elif mode == 1:
            bits = self.lib.orc_encode_block_cbr(C.byref(self.st), dst, sp, p0)
        else:
            bits = self.lib.orc_encode_block_abr(C.byref(self.st), dst, sp, p0, p1)
        ranks = np.ctypeslib.as_array(self.st.TransformIndex, (self.cb,)).copy()
        nout = self.st.lastNOutCoef
        return dict(bytes=self.tmp[:bits // 8].copy(), bits=bits, wc=self.st.WindowCtrl, cplx=np.float32(self.st.BlockComplexity),
                    nout=nout, keep=(ranks < nout).astype(np.uint8))


def oracle_streams(pcm, block_size, rate_hz, schedule):
    """pcm [B][n][C]; schedule [call][B] settings, each call covering K = n / (calls * BlockSize) blocks.
    Returns per (stream, block) lists of the oracle's per-block results."""
    B, n, ch = pcm.shape
    calls = len(schedule)
    K = n // (calls * block_size)
    res = []
    for s in range(B):
        o = OracleStream(ch, block_size, rate_hz)
        blocks = []
        for j in range(calls):
            for k in range(K):
                kk = j * K + k
                blocks.append(o.block(pcm[s, kk * block_size:(kk + 1) * block_size], schedule[j][s]))
        o.close()
        res.append(blocks)
    return res
