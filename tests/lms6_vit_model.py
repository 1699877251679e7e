"""A plain numpy model of what `lms6Xmod --vit | --vit2` does with one block of raw soft values (demod/mod/lms6Xmod.c: vit_initCodes :208-230, vit_dist2 /
vit_start / vit_next / vit_path / viterbi :232-341, deconv :345-376, proc_frame's cut at the error index :874, bits2bytes :415-441), and of the soft-bit framer
in front of it (find_softbinhead / corr_softhdb, demod_mod.c:1692-1762; main's block loop :1376-1426).  Written from the reference's description of the
operation, one array element per trellis state, no wavefront in sight: the tests hold csrc/sonde_vit_dev.h (emulated and on the device) against it byte for
byte.  It is itself pinned to the host tier and the compiled reference by tests/test_softin_lms6_emu.py::test_model_*.

Arithmetic: the branch metric is `(c0 - sb0) * (c0 - sb0) + (c1 - sb1) * (c1 - sb1)` in float, every product and sum rounded to float32 on its own (numpy
rounds after every array operation); path metrics are float32 sums.  Values that are not finite are outside the model (the reference's first-minimum loop and
its `<=` give no defined answer for NaN)."""
import numpy as np

F32 = np.float32
K = 7                        # constraint length: 64 states, 128 code words
POLY_A, POLY_B = "1001111", "1101101"
BLOCKSTART = 80
RAWBLK6, RAWBLKX = 261 * 16, 300 * 16
BB_LEN = 308
RAW_HEADER = "0101011000001000" "0001110010010111" "0001101010100111" "0011110100111110"
BLK_SYNCBITS = "0000000000000000" "0000001101011101" "0100100111000010" "0100111111110010" "0110100001101011"


def _codes():
    code = np.zeros(128, np.int64)
    for bits in range(128):
        ca = cb = 0
        for i in range(K):
            ca ^= (int(POLY_A[K - 1 - i]) & 1) & ((bits >> i) & 1)
            cb ^= (int(POLY_B[K - 1 - i]) & 1) & ((bits >> i) & 1)
        code[bits] = (ca << 1) | cb
    return code


CODE = _codes()
_C0 = (2 * ((CODE >> 1) & 1) - 1).astype(F32)
_C1 = (2 * (CODE & 1) - 1).astype(F32)
_PREV = np.arange(128) >> 1


def viterbi(sb):
    """sb[0 .. len): the path's code bits (2 * (len // 2) of them, 0 / 1) and the number of steps at which some state's two candidates had equal metrics"""
    sb = np.asarray(sb, F32)
    tmax = len(sb) // 2
    assert tmax >= K - 1
    w = np.zeros(64, F32)                                   # state[0][0].w = 0; the others do not exist yet
    second = np.zeros((tmax, 64), bool)                     # the candidate from the upper predecessor (j / 2 + 32) was kept
    ties = 0
    for t in range(tmax):
        s0, s1 = sb[2 * t], sb[2 * t + 1]
        d = (_C0 - s0) * (_C0 - s0) + (_C1 - s1) * (_C1 - s1)
        if t < K - 1:                                       # vit_start: 2^(t+1) states, one predecessor each
            m = 2 << t
            nw = np.zeros(64, F32)
            nw[:m] = w[_PREV[:m]] + d[:m]
            w = nw
        else:                                               # vit_next: candidate n = 2 j + b comes from state j; new state n % 64 keeps d[j] when d[j].w <= d[j + 64].w
            cand = w[_PREV] + d
            lo, hi = cand[:64], cand[64:]
            keep_lo = lo <= hi
            ties += bool(np.any(lo == hi))
            second[t] = ~keep_lo
            w = np.where(keep_lo, lo, hi)
    # the first minimum in ascending state order
    j, wmin = 0, w[0]
    for k in range(1, 64):
        if w[k] < wmin:
            wmin, j = w[k], k
    raw = np.zeros(2 * tmax, np.uint8)
    for t in range(tmax, 0, -1):
        n = j + 64 * int(second[t - 1][j])
        c = CODE[n]
        raw[2 * t - 2] = (c >> 1) & 1
        raw[2 * t - 1] = c & 1
        j = n >> 1
    return raw, ties


def deconv(raw):
    """the algebraic inverse over hard code bits, six zero bits assumed in front -> (characters, error index)"""
    m = K - 1
    pa, pb = [int(c) for c in POLY_A], [int(c) for c in POLY_B]
    bits = [ord("0")] * m
    n, errors = 0, 0
    while 2 * (m + n) < len(raw):
        a = b = 0
        for j in range(m):
            a ^= (bits[n + j] & 1) & pa[j]
            b ^= (bits[n + j] & 1) & pb[j]
        a ^= int(raw[2 * (m + n)]) & 1
        b ^= int(raw[2 * (m + n) + 1]) & 1
        if a == pa[m] and b == pb[m]:
            bits.append(ord("1"))
        elif a == 0 and b == 0:
            bits.append(ord("0"))
        else:
            errors = n
            break
        n += 1
    # (the character of the failing step, '8' or '9', is overwritten by the terminator: bits[n + m] = 0)
    return bits[:n + m], errors


def bits2bytes(chars):
    n = len(chars) // 8
    out = np.zeros(BB_LEN, np.uint8)
    for b in range(n):
        v = 0
        for i in range(8):
            if chars[8 * b + i] in (ord("1"), ord("9")):
                v += 1 << i
        out[b] = v
    return out, n


def decode_block(sb, with_ties=False):
    """One block sb[0 .. len) as blk_rawbits[].sb holds it (sync positions included) -> (bytes[308], blen, err)"""
    raw, ties = viterbi(sb)
    chars, err = deconv(raw)
    if err:
        chars = chars[:err]                                  # proc_frame: the string ends at the error index
    by, blen = bits2bytes(chars)
    return (by, blen, err, ties) if with_ties else (by, blen, err)


def sync_sb():
    return np.array([2 * (ord(c) & 1) - 1 for c in BLK_SYNCBITS], F32)


def block_sb(raw_soft, mv, vit):
    """main's block loop: the soft values behind a header (raw polarity) -> blk_rawbits[].sb, the 80 sync positions in front"""
    s = np.asarray(raw_soft, F32)
    bc = (0 if mv > 0 else 1) + np.arange(len(s))
    odd = bc % 2
    hb = (s >= 0).astype(np.int64) ^ odd
    sb = ((-2 * odd + 1).astype(F32) * s).astype(F32)
    if vit == 1:
        sb = (2 * hb - 1).astype(F32)
    return np.concatenate([sync_sb(), sb])


def header_score(win):
    """corr_softhdb over 64 soft values, oldest first: float products, double sums in order"""
    win = np.asarray(win, F32)
    y = np.array([2.0 * (ord(c) & 1) - 1.0 for c in RAW_HEADER], F32)
    s = nx = 0.0
    for k in range(64):
        s += float(F32(y[k] * win[k]))
        nx += float(F32(win[k] * win[k]))
    with np.errstate(all="ignore"):
        return F32(np.float64(s) / np.sqrt(np.float64(nx) * 64.0))


def frame_stream(soft, next_len, invert=False):
    """find_softbinhead + the block loop over a whole stream: [(hdr_bit, mv, raw soft values of the block)] for every COMPLETE block.  next_len(k) = raw bits
    read behind the header of block k (4096 or 4720).  hdr_bit = index of the first soft bit behind the header.  The ring only moves while searching."""
    x = np.asarray(soft, F32)
    if invert:
        x = -x
    y = np.array([2.0 * (ord(c) & 1) - 1.0 for c in RAW_HEADER], np.float64)
    ring = np.zeros(64, F32)
    cur, out = 0, []
    while cur < len(x):
        hit = None
        while cur < len(x) and hit is None:
            seg = np.concatenate([ring[1:], x[cur:cur + 4096]])              # window i = seg[i : i + 64] ends at stream position cur + i
            win = np.lib.stride_tricks.sliding_window_view(seg, 64)
            with np.errstate(all="ignore"):
                est = (win.astype(np.float64) @ y) / np.sqrt((win.astype(np.float64) ** 2).sum(axis=1) * 64.0)
            for i in np.nonzero(np.abs(est) > 0.69)[0]:                      # (the decision itself: the reference's arithmetic)
                mv = header_score(win[i])
                if abs(float(mv)) > float(F32(0.7)):
                    hit = (int(i), mv, win[i].copy())
                    break
            if hit is None:
                n = min(4096, len(x) - cur)
                ring = np.concatenate([ring, x[cur:cur + n]])[-64:]
                cur += n
        if hit is None:
            break
        i, mv, ring = hit
        start = cur + i + 1
        n = next_len(len(out))
        if start + n > len(x):
            break
        out.append((start, mv, x[start:start + n].copy()))
        cur = start + n
    return out


# ---- the streams the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------
def soft_stream(n_blocks, lmsx=False, sigma=0.0, seed=1, lead=37, invert=False, grid=False, erase=0.0, tail=200):
    """n_blocks on-air blocks as +-1 behind `lead` noise samples, Gaussian noise of `sigma` on everything, optionally rounded to a 0.5 grid, with a share
    `erase` of exact zeros, negated; then `tail` noise samples in which the last block completes and no header is found"""
    from tools import synth
    bits = synth.lms6_onair_bits(n_blocks, lmsx)
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.normal(0, 0.3, lead), 2.0 * bits.astype(np.float64) - 1.0])
    s = s + rng.normal(0.0, sigma, len(s))
    if grid:
        s = np.round(2.0 * s) / 2.0
    if erase:
        s[rng.random(len(s)) < erase] = 0.0
    if invert:
        s = -s
    s = np.concatenate([s, np.random.default_rng(1000 + seed).normal(0, 0.3, tail)])
    return s.astype(F32)


# kind -> (vit, keyword arguments of soft_stream)
NOISY_KINDS = {
    "vit_s07": (1, dict(sigma=0.7)),
    "vit2_s09": (2, dict(sigma=0.9)),
    "grid": (2, dict(sigma=0.8, grid=True)),
    "erased": (2, dict(sigma=0.75, erase=0.15)),
    "inverted": (1, dict(sigma=0.7, invert=True)),
}
# type -> (typ option, LMS-X blocks, reference option)
NOISY_TYPES = {"lms6": (6, False, ["--lms6"]), "lmsx": (10, True, ["--lmsX"]), "auto": (0, False, [])}
# (seeds: 100 + 10 * type + kind, except where that stream gave the host tier fewer than three frame lines at sigma 0.9)
NOISY_SEEDS = {("lms6", "vit2_s09"): 201, ("lmsx", "vit2_s09"): 200}


def noisy_stream(typ_name, kind, n_blocks=4, lead=37):
    """-> (stream, its noiseless counterpart, typ, vit, reference options)"""
    typ, lmsx, ropt = NOISY_TYPES[typ_name]
    vit, kw = NOISY_KINDS[kind]
    seed = NOISY_SEEDS.get((typ_name, kind), 100 + 10 * list(NOISY_TYPES).index(typ_name) + list(NOISY_KINDS).index(kind))
    s = soft_stream(n_blocks, lmsx, seed=seed, lead=lead, **kw)
    clean = soft_stream(n_blocks, lmsx, seed=seed, lead=lead, invert=kw.get("invert", False))
    return s, clean, typ, vit, ropt + ["--vit" if vit == 1 else "--vit2"]


def threshold_stream(flips, target=None, invert=False, seed=7, lead=37):
    """One clean +-1 LMS6 block whose 64 header bits (positions 16 .. 79 of the block) carry `flips` sign errors: score (64 - 2 flips) / 64.  With a target, the
    header values get 5 % amplitude noise and the flipped ones a common factor found by bisection, so that corr_softhdb's value lands on the target.
    -> (stream, score of the header window as header_score computes it, hdr_bit of the block)"""
    from tools import synth
    rng = np.random.default_rng(seed)
    s = 2.0 * synth.lms6_onair_bits(1).astype(np.float64) - 1.0
    at = 16 + rng.choice(64, flips, replace=False)
    s[at] = -s[at]
    if target is not None:
        s[16:80] *= 1.0 + 0.05 * rng.normal(0, 1, 64)
        base = s.copy()
        lo, hi = 0.3, 2.0                                       # the score falls as the flipped values grow
        for _ in range(60):
            m = 0.5 * (lo + hi)
            s = base.copy()
            s[at] *= m
            if float(header_score(s[16:80].astype(F32))) > target:
                lo = m
            else:
                hi = m
    s = np.concatenate([rng.normal(0, 0.3, lead), s, rng.normal(0, 0.3, 200)])
    if invert:
        s = -s
    s = s.astype(F32)
    return s, float(header_score(-s[lead + 16:lead + 80] if invert else s[lead + 16:lead + 80])), lead + 80


# name -> (flips, target score or None)
THRESHOLD_CASES = {"9_flips": (9, None), "10_flips": (10, None), "9_flips_above": (9, 0.7004), "9_flips_below": (9, 0.6996),
                   "10_flips_above": (10, 0.7004), "10_flips_below": (10, 0.6996)}
