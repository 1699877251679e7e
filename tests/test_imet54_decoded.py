"""sonde_imet54_dec_decoded (include/sonde_imet54.h): the text of a complete iMet-54 frame that is decoded already — what the device consumer hands over per frame
(tests/test_gpu_softin_imet54.py).  The arbiter is the host tier itself: sonde_imet54_dec_frame on the frame's 2200 soft bits prints the text, its `-r --ecc` line
gives the 108 bytes, the ecc sums and the tag, and the new entry, fed those values, must print the same text under every option set.  It prints from the values it
is given: a verdict that contradicts the bytes shows in the text."""
import ctypes as C

import numpy as np
import pytest

import imet54_softin_cases as M

OPTS = {"-r": dict(raw=1), "-r --ecc": dict(raw=1, ecc=1), "-r4 --ecc": dict(raw=4, ecc=1), "plain": dict(), "--ecc": dict(ecc=1), "-v --ptu --ecc": dict(verbose=1, ptu=1, ecc=1),
        "--json --ptu": dict(json=1, ptu=1, version="t", jsn_freq_khz=402300), "-r --json --ptu": dict(raw=1, json=1, ptu=1), "--silent --json": dict(silent=1, json=1)}


@pytest.fixture(scope="module")
def host():
    return M.load_host()


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


def _frames():
    """name -> 2200 frame bits: every tag, repaired and uncorrectable codewords, an iMet-50, a frame whose GPS fields are out of range"""
    H, S = M.hamming_bits(), M.checksum_bits()
    c = {k: H[k][0] for k in ("no_error", "one_flip_each", "two_flips", "f0_at_87", "f0_at_88", "f0_at_104")}
    c.update({k: S[k][0] for k in ("check_std", "check_cont", "check_none", "none_f8_repaired", "none_not_f8_repaired", "check_cont_flip52", "check_std_flip0")})
    c["imet50"] = M.fbits(M.frame(2, imet50=True))
    f = bytearray(M.frame(2, check="cont")); f[8] = 0x7F
    c["gps_out_of_range"] = M.fbits(bytes(f))
    return c


def _text(host, d, bits):
    sb = np.ascontiguousarray(2.0 * np.asarray(bits, np.float32) - 1.0, np.float32)
    buf = C.create_string_buffer(4096)
    n = host.sonde_imet54_dec_frame(d, sb.ctypes.data, 2200, buf, 4096)
    assert n >= 0
    return buf.raw[:n].decode()


def _decoded(host, d, fr, frm, tlm, std, crc_std, crc_cont, size=4096):
    buf = C.create_string_buffer(size)
    n = host.sonde_imet54_dec_decoded(d, fr, frm, tlm, std, crc_std, crc_cont, buf, size)
    return n, buf.raw[:max(n, 0)].decode()


@pytest.mark.parametrize("opt", sorted(OPTS))
def test_decoded_reproduces_the_arbiters_text(host, emu, opt):
    o = OPTS[opt]
    ecc = 1 if o.get("ecc") or o.get("json") else 0
    tags = set()
    for name, bits in _frames().items():
        raw = M.host_dec(host, raw=1, ecc=ecc)
        fr, frm, tlm, tag = M.parse_raw_line(_text(host, raw, bits).rstrip("\n"), ecc)
        host.sonde_imet54_dec_destroy(raw)
        if not ecc:                                              # (without --ecc the line has no sums: those of the emulated end-of-frame step, which
            r = M.Rec()                                          # tests/test_softin_imet54_emu.py pins to the same arbiter)
            assert emu.emu_imet54_end(M.chars_of(bits), 0, C.byref(r)) == 0 and bytes(r.frame) == fr and M.tag_of(r) == tag
            frm, tlm = r.ecc_frm, r.ecc_tlm
        tags.add(tag)
        a, b = M.host_dec(host, **o), M.host_dec(host, **o)
        want = _text(host, a, bits)
        n, got = _decoded(host, b, fr, frm, tlm, frm, int(tag == "[OK]"), int(tag == "[ok]"))
        assert n == len(want) and got == want, (opt, name)
        host.sonde_imet54_dec_destroy(a); host.sonde_imet54_dec_destroy(b)
    if ecc:
        assert tags == {"[OK]", "[ok]", "[oo]", "[NO]", "[no]"}


def test_decoded_prints_from_the_values_it_is_given(host):
    fr = M.frame(4, check="none")
    d = M.host_dec(host, raw=1, ecc=1)
    line = lambda *v: _decoded(host, d, fr, *v)[1].rstrip("\n")   # noqa: E731
    hexs = fr.hex().upper()
    assert line(0, 0, 0, 0, 0) == hexs + " [oo]"
    assert line(0, 0, 0, 1, 0) == hexs + " [OK]"                  # neither check sum is computed again
    assert line(0, 0, 0, 0, 1) == hexs + " [ok]"
    assert line(3, 2, 3, 0, 0) == hexs + " [NO] # (3) [2]"
    assert line(-1, 1, -1, 0, 1) == hexs + " [ok] # (-1) [1]"
    g = bytearray(fr); g[0x52] = 0
    assert _decoded(host, d, bytes(g), -1, -1, -1, 0, 0)[1].rstrip("\n") == bytes(g).hex().upper() + " [no] # (-1) [-1]"
    host.sonde_imet54_dec_destroy(d)
    # the JSON rule: frm_ok and a check sum (or ecc_std == 0), status bits 0x30
    d = M.host_dec(host, json=1, ptu=1)
    assert '"type": "IMET5"' in _decoded(host, d, fr, 0, 0, 0, 0, 0)[1]           # [oo]
    assert '"type": "IMET5"' not in _decoded(host, d, fr, 2, 2, 2, 0, 0)[1]       # [NO]
    assert '"type": "IMET5"' in _decoded(host, d, fr, 2, 2, 2, 0, 1)[1]
    assert '"type": "IMET5"' not in _decoded(host, d, fr, -1, 2, -1, 1, 0)[1]
    host.sonde_imet54_dec_destroy(d)


def test_decoded_leaves_the_existing_entries_alone_and_checks_its_arguments(host):
    """a decoder that printed a decoded frame goes on computing both check sums itself; bad arguments and a short buffer are SONDE_E_ARG"""
    d = M.host_dec(host, raw=1, ecc=1)
    fr = M.frame(4, check="none")
    assert _decoded(host, d, fr, 0, 0, 0, 1, 0)[1].endswith("[OK]\n")
    assert _text(host, d, M.fbits(M.frame(5, check="cont"))).rstrip("\n").endswith("[ok]")
    assert _text(host, d, M.fbits(fr)).rstrip("\n").endswith("[oo]")
    assert host.sonde_imet54_dec_decoded(None, fr, 0, 0, 0, 0, 0, C.create_string_buffer(8), 8) == -1
    assert host.sonde_imet54_dec_decoded(d, None, 0, 0, 0, 0, 0, C.create_string_buffer(8), 8) == -1
    assert host.sonde_imet54_dec_decoded(d, fr, 0, 0, 0, 0, 0, None, 8) == -1
    assert _decoded(host, d, fr, 0, 0, 0, 0, 0, size=100)[0] == -1
    host.sonde_imet54_dec_destroy(d)
