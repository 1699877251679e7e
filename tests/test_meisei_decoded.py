"""sonde_meisei_dec_decoded (include/sonde_meisei.h): the text of a complete Meisei frame that is decoded already — what the device consumer hands over per frame
(tests/test_gpu_softin_meisei.py).  The arbiter is the host tier itself: sonde_meisei_dec_push_soft over a stream prints the text, its frames give the 600 bits and
the 12 block verdicts (meisei_softin_cases.host_frames, which pins them to the `-r --ecc -v` line), and the new entry, fed those values frame by frame, must print
the same text under every option set — across a type hand-over from RS-11G to iMS-100 and back and over a full 64-frame configuration cycle.  It prints from the
values it is given: a verdict that contradicts the bits shows in the text."""
import ctypes as C

import numpy as np
import pytest

import meisei_softin_cases as M

OPTS = {"-r": dict(raw=1), "-r --ecc -v": dict(raw=1, ecc=1, verbose=1), "--ecc": dict(ecc=1), "--ecc -v --ptu": dict(ecc=1, verbose=1, ptu=1),
        "--json --ptu --ecc": dict(json=1, ptu=1, ecc=1, version="t", jsn_freq_khz=404500), "--ims100 --json": dict(ims100=1, json=1),
        "--rs11g --ecc --ptu": dict(ecc=1, ptu=1), "--year 2035 --json": dict(ref_year=2035, json=1), "--dbg": dict(dbg=1)}


@pytest.fixture(scope="module")
def host():
    return M.load_host()


_stream = {}


def _hand_over_stream():
    """4 RS-11G frames, 68 iMS-100 frames (more than the 64-frame configuration cycle), 4 RS-11G frames, continuous; single and double bit errors in some blocks
    and three frames with a block beyond repair"""
    if "s" not in _stream:
        sym = np.concatenate([M.fsym(0, "rs11g", 4), M.fsym(4, "ims100", 68), M.fsym(72, "rs11g", 4)])
        # (each part starts on a low level: where the part before it ended high, the stream jumps — the header search does not mind)
        s = M.soft(sym)
        rng = np.random.default_rng(11)
        for fr in (1, 6, 9, 20, 33, 50, 70, 74):                 # one or two flipped bits in three blocks
            for blk in rng.choice(12, 3, replace=False):
                for j in rng.choice(46, int(rng.integers(1, 3)), replace=False):
                    s[1200 * fr + 2 * (M.block_at(int(blk)) + int(j))] *= -1
        for fr in (12, 41, 73):                                  # five flipped bits in one block
            for j in rng.choice(46, 5, replace=False):
                s[1200 * fr + 2 * (M.block_at(int(fr % 12)) + int(j))] *= -1
        _stream["s"] = np.concatenate([s, np.zeros(40, np.float32)])
    return _stream["s"]


def _decoded(host, d, bits, be, size=4096):
    buf = C.create_string_buffer(size)
    n = host.sonde_meisei_dec_decoded(d, bytes(bits), bytes(be), buf, size)
    return n, buf.raw[:max(n, 0)].decode()


@pytest.mark.parametrize("opt", sorted(OPTS))
def test_decoded_reproduces_the_arbiters_text(host, opt):
    o = OPTS[opt]
    ecc = 1 if o.get("ecc") or o.get("json") else 0
    s = _hand_over_stream()
    frames = M.host_frames(host, s, ecc=ecc, cache="handover%d" % ecc)
    assert len(frames) == 76
    if ecc:
        seen = set(v for f in frames for v in f[2])
        assert {0, 1, 2} <= seen and (0xE in seen or 0xF in seen)
    want = M.host_text(host, s, **o)
    d = M.host_dec(host, **o)
    got = ""
    for _, bits, be, _ in frames:
        n, t = _decoded(host, d, bits, be)
        assert n == len(t) and n >= 0
        got += t
    host.sonde_meisei_dec_destroy(d)
    assert got == want, opt
    if o.get("json"):
        assert got.count('"id": "IMS100-') > 20 and got.count('"id": "RS11G-') >= 1 if not o.get("ims100") else got.count('"type": "MEISEI"') > 20
    if not o.get("raw"):
        assert got.count("\n") > 76


def test_decoded_prints_from_the_values_it_is_given(host):
    """a verdict that contradicts the bits: [NO] on clean bits, and the raw line shows the verdicts given"""
    ok = bytes(12)
    d = M.host_dec(host, ecc=1, ims100=1)
    a = _decoded(host, d, M.pack(M.frame_bits(4)), ok)[1]
    b = _decoded(host, d, M.pack(M.frame_bits(6)), bytes([0, 0, 0xE] + [0] * 9))[1]
    assert "[OK]" in a and "[NO]" not in a and "[NO]" in b and "[OK]" not in b
    host.sonde_meisei_dec_destroy(d)
    d = M.host_dec(host, raw=1, ecc=1, verbose=1)
    be = bytes([0, 1, 2, 0xE, 0xF, 0, 2, 1, 0, 0xF, 0xE, 1])
    line = _decoded(host, d, M.pack(M.frame_bits(4)), be)[1]
    assert line == M.raw_line((0, M.pack(M.frame_bits(4)), be), 1) + "\n" and "#012EF0#" in line and "#210FE1#" in line
    host.sonde_meisei_dec_destroy(d)
    # without --ecc the verdicts are not looked at
    d = M.host_dec(host, raw=1, verbose=1)
    assert _decoded(host, d, M.pack(M.frame_bits(4)), be)[1] == M.raw_line((0, M.pack(M.frame_bits(4)), be), 0) + "\n"
    host.sonde_meisei_dec_destroy(d)


def test_decoded_leaves_the_existing_entries_alone_and_checks_its_arguments(host):
    """a decoder that printed a decoded frame goes on decoding its own blocks in sonde_meisei_dec_frame; bad arguments and a short buffer are SONDE_E_ARG"""
    d = M.host_dec(host, raw=1, ecc=1, verbose=1)
    bits = M.pack(M.frame_bits(4))
    assert "#EEEEEE#" in _decoded(host, d, bits, bytes([0xE] * 12))[1]
    sb = np.ascontiguousarray(M.soft(M.fsym(4))[48:], np.float32)
    buf = C.create_string_buffer(1024)
    n = host.sonde_meisei_dec_frame(d, sb.ctypes.data, 1152, buf, 1024)
    assert buf.raw[:n].decode() == M.raw_line((0, bits, bytes(12)), 1) + "\n"
    assert host.sonde_meisei_dec_decoded(None, bits, bytes(12), C.create_string_buffer(8), 8) == -1
    assert host.sonde_meisei_dec_decoded(d, None, bytes(12), C.create_string_buffer(8), 8) == -1
    assert host.sonde_meisei_dec_decoded(d, bits, None, C.create_string_buffer(8), 8) == -1
    assert host.sonde_meisei_dec_decoded(d, bits, bytes(12), None, 8) == -1
    assert _decoded(host, d, bits, bytes(12), size=50)[0] == -1
    host.sonde_meisei_dec_destroy(d)
