"""A float64 referee for the codec's transform path, written from the reference's normative FormatSpecs.md ALONE (no
libulc source, no oracle code, no lapping buffers): header table (FormatSpecs.md:33-55), IMDCT and sine window
(:150-155), overlap clipping (:157).  Test infrastructure (tests/test_transform_referee.py,
tests/test_gpu_transform_referee.py).

Everything lives on one global timeline of samples.  For block b (0-based here; 1-based b+1 in the issue's wording):

  * sub-blocks S_0, S_1, ... from the header table; sub-block j owns the transition T_j = T_0 + sum_{i<j} S_i, and its
    frame is the 2 S_j samples starting at T_j - S_j/2 (so its right half is centred on T_{j+1});
  * decoder (output axis, output block b = samples [b N, (b+1) N)):  T_0 = b N + N/2;
    encoder (input axis):                                             T_0 = (b-2) N + N/2, input before sample 0 is zero.
    The round trip therefore delays by 2 N;
  * overlap at transition j: S_j, shifted right by the header's scale when sub-block j carries the asterisk, then clipped
    to S_{j-1} (which may be the previous block's last sub-block).  A stream's first transition has S_{-1} = 0, i.e.
    overlap 0;
  * coefficients X[k] = -(2/S) sum_n f[n] cos(pi/S (n + 1/2 + S/2)(k + 1/2)), f = windowed frame; synthesis is the spec's
    IMDCT y[n] = -sum_k X[k] cos(pi/S (n + 1/2 + S/2)(k + 1/2)) (no 2/S), windowed and added in;
  * M/S over channel pairs (0,1), (2,3), ...: the encoder transforms M = (L+R)/2, S = (L-R)/2, the decoder outputs
    L = M+S, R = M-S.

Window at a transition T with overlap ov (rise for the frame on the right of T, fall = its mirror image about T for the
frame on the left: fall(T-1-i) = rise(T+i)):
  ov = 0        hard step: rise(t) = [t >= T];
  ov even >= 2  sine ramp on [T - ov/2, T + ov/2): rise(T - ov/2 + i) = sin(pi/2 (i + 1/2) / ov);
  ov = 1        (a 128-sample sub-block at scale 7, 64 at 6, 32 at 5: the decoder must accept these although no encoder
                writes overlaps below 32)  the spec's ramp would be half a sample wide and centred on T - 1/2, which no
                sample is.  Convention: the two samples that straddle T form one butterfly at pi/4,
                rise(T-1) = rise(T) = fall(T-1) = fall(T) = sin(pi/4); 0 / 1 outside.  This keeps time-domain alias
                cancellation exact (fall(t) fall(t') = rise(t) rise(t') for the mirror pair, fall^2 + rise^2 = 1).
                A plain sine ramp started at sample T - 1 (rise = sin(pi/4) there and 1 from T on) is NOT this
                convention and does not reconstruct.

Each transform has two evaluations: a direct O(S^2) sum and a numpy FFT of 2 S points (both binary64);
method="auto" takes the direct sum for S <= DIRECT_MAX.
"""
import numpy as np

DIRECT_MAX = 256
_S4 = np.sin(np.pi / 4)

# FormatSpecs.md:35-51 - second header nybble -> (sub-block sizes as divisors of N, index of the asterisk sub-block)
HEADER_TABLE = {
    0b0010: ((2, 2), 0), 0b0011: ((2, 2), 1),
    0b0100: ((4, 4, 2), 0), 0b0101: ((4, 4, 2), 1), 0b0110: ((2, 4, 4), 1), 0b0111: ((2, 4, 4), 2),
    0b1000: ((8, 8, 4, 2), 0), 0b1001: ((8, 8, 4, 2), 1), 0b1010: ((4, 8, 8, 2), 1), 0b1011: ((4, 8, 8, 2), 2),
    0b1100: ((2, 8, 8, 4), 1), 0b1101: ((2, 8, 8, 4), 2), 0b1110: ((2, 4, 8, 8), 2), 0b1111: ((2, 4, 8, 8), 3),
}


def header_code(wc):
    """A block's header as (first nybble, second nybble or None): the codec's WindowCtrl word keeps the first nybble in
    bits 0-3 and, for a decimated block, the second in bits 4-7."""
    wc = int(wc)
    first = wc & 15
    return (first, (wc >> 4) & 15) if first & 8 else (first, None)


def geometry(wc, N, reverse=False):
    """-> (sizes, nominal overlaps) of one header, before clipping: ov_j = S_j >> scale on the asterisk sub-block, S_j
    elsewhere.  reverse: the table read backwards (a wrong reading, for the sensitivity tests)."""
    first, second = header_code(wc)
    scale = first & 7
    if second is None:
        sizes, star = [N], 0
    else:
        if second not in HEADER_TABLE:
            raise ValueError("header %#x is outside FormatSpecs.md's table" % wc)
        divs, star = HEADER_TABLE[second]
        sizes = [N // d for d in divs]
    ovs = [S >> scale if j == star else S for j, S in enumerate(sizes)]
    if reverse:
        sizes, ovs = sizes[::-1], ovs[::-1]
    return sizes, ovs


def layout(wcs, N, origin, clip=True, reverse=False, shift=0):
    """Frames of a block sequence: per block a list of (T, S, ovL, ovR) - transition on the frame's left, size, overlap at
    T and at T + S.  origin: the first transition of block 0 is at origin + N/2.  The last block's right overlap is not
    known (it belongs to the next header) and is given as its own size; only samples before the last block's end
    transition are complete."""
    blocks = []
    prev = 0
    for b, wc in enumerate(wcs):
        sizes, ovs = geometry(wc, N, reverse)
        T = origin + b * N + N // 2 + shift
        row = []
        for S, ov in zip(sizes, ovs):
            if clip:
                ov = min(ov, prev)
            row.append([T, S, ov, None])
            prev = S
            T += S
        blocks.append(row)
    flat = [f for row in blocks for f in row]
    for f, g in zip(flat, flat[1:]):
        f[3] = g[2]
    flat[-1][3] = flat[-1][1]
    return [[tuple(f) for f in row] for row in blocks]


def rise(d, ov, plain_ov1=False):
    """Rising window at distance d = t - T from a transition (t the sample index).  plain_ov1: a plain sine ramp started at
    T - 1 for ov = 1 instead of the butterfly (a wrong reading, for the sensitivity tests)."""
    d = np.asarray(d, np.float64)
    if ov == 0:
        return (d >= 0).astype(np.float64)
    if ov == 1:
        if plain_ov1:
            return np.where(d < -1, 0.0, np.where(d < 0, _S4, 1.0))
        return np.where(d < -1, 0.0, np.where(d < 1, _S4, 1.0))
    u = np.clip((d + ov / 2 + 0.5) / ov, 0.0, 1.0)
    return np.sin(np.pi / 2 * u)


def fall(d, ov, plain_ov1=False):
    """Falling window at distance d = t - T: the mirror image of rise about T (fall(T-1-i) = rise(T+i)); for the plain
    ov = 1 ramp the complement cos of the same ramp."""
    if ov == 1 and plain_ov1:
        d = np.asarray(d, np.float64)
        return np.where(d < -1, 1.0, np.where(d < 0, _S4, 0.0))
    return rise(-1 - np.asarray(d), ov)


def frame_window(T, S, ovL, ovR, plain_ov1=False):
    t = np.arange(T - S // 2, T + 3 * S // 2)
    return rise(t - T, ovL, plain_ov1) * fall(t - (T + S), ovR, plain_ov1)


# ---- the two transforms, batched over rows ---------------------------------------------------------------------------
def _basis(S):
    """cos(pi/S (n + 1/2 + S/2)(k + 1/2)) = cos(pi m / 4S), m = (2n + 1 + S)(2k + 1) reduced mod 8S in integers (no
    rounding of large arguments)."""
    n = np.arange(2 * S, dtype=np.int64)[:, None]
    k = np.arange(S, dtype=np.int64)[None, :]
    m = ((2 * n + 1 + S) * (2 * k + 1)) % (8 * S)
    return np.cos(np.pi * m / (4 * S))                      # [2S][S]


def mdct(f, method="auto"):
    """f [..., 2S] -> X [..., S], X[k] = -(2/S) sum_n f[n] cos(pi/S (n + 1/2 + S/2)(k + 1/2))."""
    f = np.asarray(f, np.float64)
    S = f.shape[-1] // 2
    if method == "direct" or (method == "auto" and S <= DIRECT_MAX):
        return -(2.0 / S) * (f @ _basis(S))
    n = np.arange(2 * S, dtype=np.int64)
    k = np.arange(S, dtype=np.int64)
    g = np.fft.fft(f * np.exp(-1j * np.pi * n / (2 * S)), axis=-1)[..., :S]
    post = ((1 + S) * (2 * k + 1)) % (8 * S)                # exp(-i pi/S (1/2 + S/2)(k + 1/2)), argument reduced in integers
    return -(2.0 / S) * np.real(np.exp(-1j * np.pi * post / (4 * S)) * g)


def imdct(X, method="auto"):
    """X [..., S] -> y [..., 2S], y[n] = -sum_k X[k] cos(pi/S (n + 1/2 + S/2)(k + 1/2))."""
    X = np.asarray(X, np.float64)
    S = X.shape[-1]
    if method == "direct" or (method == "auto" and S <= DIRECT_MAX):
        return -(X @ _basis(S).T)
    n = np.arange(2 * S, dtype=np.int64)
    k = np.arange(S, dtype=np.int64)
    h = np.zeros(X.shape[:-1] + (2 * S,), np.complex128)
    h[..., :S] = X * np.exp(1j * np.pi * (((1 + S) * k) % (4 * S)) / (2 * S))      # exp(i pi/S (1/2 + S/2) k), reduced
    H = np.fft.ifft(h, axis=-1) * (2 * S)
    return -np.real(np.exp(1j * np.pi * (2 * n + 1 + S) / (4 * S)) * H)


def ms_fold(pcm):
    """[n][C] -> M/S over channel pairs (0,1), (2,3), ...: M = (L+R)/2, S = (L-R)/2."""
    x = np.array(pcm, np.float64)
    for c in range(1, x.shape[1], 2):
        l, r = x[:, c - 1].copy(), x[:, c].copy()
        x[:, c - 1], x[:, c] = (l + r) / 2, (l - r) / 2
    return x


def ms_unfold(y):
    y = np.array(y, np.float64)
    for c in range(1, y.shape[1], 2):
        m, s = y[:, c - 1].copy(), y[:, c].copy()
        y[:, c - 1], y[:, c] = m + s, m - s
    return y


def _groups(frames):
    """frames: iterable of (block, T, S, ovL, ovR, offset within the channel's coefficients) -> {S: [...]}"""
    g = {}
    for fr in frames:
        g.setdefault(fr[2], []).append(fr)
    return g


def analyse(pcm, wc, N, method="auto", **wrong):
    """pcm [n][C] (one stream; n a multiple of N), wc [K] the headers the encoder wrote for its K blocks ->
    coefficients [K-1][C*N] of every block whose successor's header is known, laid out as the codec's coefficient tap
    (channel-major, sub-blocks in header order).  wrong: clip / reverse / shift / plain_ov1, for the sensitivity tests."""
    x = ms_fold(pcm)
    n, C = x.shape
    K = len(wc)
    plain = wrong.pop("plain_ov1", False)
    lay = layout(wc, N, origin=-2 * N, **wrong)
    out = np.zeros((K - 1, C, N))
    frames = []
    for b in range(K - 1):
        off = 0
        for (T, S, ovL, ovR) in lay[b]:
            frames.append((b, T, S, ovL, ovR, off))
            off += S
    for S, fr in _groups(frames).items():
        idx = np.array([f[1] - S // 2 for f in fr])[:, None] + np.arange(2 * S)[None, :]      # [F][2S] sample indices
        ok = (idx >= 0) & (idx < n)
        seg = np.where(ok[..., None], x[np.clip(idx, 0, n - 1)], 0.0)                         # [F][2S][C]
        w = np.stack([frame_window(f[1], S, f[3], f[4], plain) for f in fr])                 # [F][2S]
        X = mdct(np.moveaxis(seg * w[..., None], 1, 2), method)                               # [F][C][S]
        for i, f in enumerate(fr):
            out[f[0], :, f[5]:f[5] + S] = X[i]
    return out.reshape(K - 1, C * N)


def synthesise(coefs, wc, N, C, method="auto", **wrong):
    """coefs [K][C*N] (the decoder's dequantised coefficients, or analyse()'s), wc the headers of those K blocks (one more
    entry, when known, gives the last block its right overlap) -> PCM [(K+1) N][C] on the decoder's output axis: output
    block b is samples [b N, (b+1) N), complete for b < K.  A stream's first transition has overlap 0."""
    coefs = np.asarray(coefs, np.float64)
    K = coefs.shape[0]
    coefs = coefs.reshape(K, C, N)
    plain = wrong.pop("plain_ov1", False)
    lay = layout(list(wc[:K + 1]), N, origin=0, **wrong)
    y = np.zeros(((K + 2) * N, C))
    frames = []
    for b in range(K):
        off = 0
        for (T, S, ovL, ovR) in lay[b]:
            frames.append((b, T, S, ovL, ovR, off))
            off += S
    for S, fr in _groups(frames).items():
        X = np.stack([coefs[f[0], :, f[5]:f[5] + S] for f in fr])                            # [F][C][S]
        w = np.stack([frame_window(f[1], S, f[3], f[4], plain) for f in fr])
        z = imdct(X, method) * w[:, None, :]                                                  # [F][C][2S]
        for i, f in enumerate(fr):
            t0 = f[1] - S // 2
            lo = max(t0, 0)
            y[lo:t0 + 2 * S] += z[i, :, lo - t0:].T
    return ms_unfold(y[:(K + 1) * N])


def unit_errors(got, ref):
    """got, ref [..., L]: one row per (stream, block, channel) unit -> max |got - ref| / max |ref| per unit.  A unit whose
    reference is all zero must come out as exact zeros: its error is 0 if it does and inf otherwise."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    peak = np.abs(ref).max(axis=-1)
    err = np.abs(got - ref).max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(peak > 0, err / np.where(peak > 0, peak, 1.0), np.where(err > 0, np.inf, 0.0))
    return rel


def pcm_units(y, N):
    """PCM [n][C] (n a multiple of N) -> [n/N][C][N], one row per (block, channel)."""
    y = np.asarray(y)
    return y.reshape(y.shape[0] // N, N, y.shape[1]).transpose(0, 2, 1)
