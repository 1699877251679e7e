"""The dropsonde printer (host code, no GPU) against the reference's rd94rd41drop: the goldens hold, for several captures, the -r lines (the
120 bytes of every frame the reference printed) and its text, -R, -v, -vv and JSON output for the same stream.  Feeding the -r bytes to the
printer must give the other outputs byte for byte — both kinds, forced and automatic type, frames with bad blocks between good ones (the
fields that persist), and frames that the reference types RD94 only through its slip."""
import numpy as np
import pytest

from tests import drop_cases as cases
from tools import synth


def _printer(argv):
    from radiosonde_auto_rx_amd.drop import DropPrinter
    cfq = int(argv[argv.index("--jsn_cfq") + 1]) if "--jsn_cfq" in argv else -1
    return DropPrinter(raw=2 if "-R" in argv else 1 if "-r" in argv else 0, vbs=2 if "-vv" in argv else 1 if "-v" in argv else 0, json="--json" in argv,
                       type=41 if "--rd41" in argv else 94 if "--rd94" in argv else 0, jsn_freq_khz=(cfq + 500) // 1000 if cfq >= 300000000 else 0,
                       version="oracle")


def _same_stream(a, b):
    """two argument lists read the same frames when they differ in output options only"""
    strip = lambda v: sorted(x for x in v if x in ("-b", "-i", "--br", "--softin", "--softinv") or x.replace(".", "").isdigit() and x != "403000000")
    return strip(a) == strip(b)


@pytest.mark.parametrize("name", sorted(n for n, c in cases.CASES.items() if c["gen"].get("form") != "rawhex"))
def test_printer_reproduces_every_output_form_from_the_r_lines(name):
    g = cases.load(name)
    checked = 0
    for i, av in enumerate(g["argv"]):
        if "-r" not in av:
            continue
        frames = [bytes.fromhex(l) for l in g["stdout"][i].decode().split("\n") if l]
        assert all(len(f) == 120 for f in frames)
        for j, aw in enumerate(g["argv"]):
            if not _same_stream([x for x in av if x != "-r"], [x for x in aw if x not in ("-r", "-R", "-v", "-vv", "--json", "--rd41", "--rd94", "--jsn_cfq")]):
                continue
            p = _printer(aw)
            text = "".join(p.frame(f) for f in frames)
            assert text.encode() == g["stdout"][j], (name, aw, text[-600:], g["stdout"][j][-600:])
            checked += 1
    if any("-r" in av for av in g["argv"]):
        assert checked >= 1


def test_rawhex_golden_and_persistent_fields():
    """--rawhex through the line helper and the printer = the reference on the same lines; the case holds good frames, frames with one bad
    block (text, no JSON) and frames with a bad block that suppresses the text"""
    from radiosonde_auto_rx_amd import drop
    case, g = cases.CASES["rawhex"], cases.load("rawhex")
    lines = cases.capture(case).split(b"\n")
    for av, ref in zip(g["argv"], g["stdout"]):
        p, prev, text = _printer(av), bytes(120), ""
        for l in lines:
            if not l:
                continue
            prev, ok = drop.rawhex(l + b"\n", prev)
            if ok:
                text += p.frame(prev)
        assert text.encode() == ref, (av, text[-500:], ref[-500:])
    assert g["stdout"][0].count(b'"type"') == 3 and g["stdout"][0].count(b"# chk: 00010") >= 1
    b, ok = drop.rawhex(b"fc1dzz01\n", bytes([9] * 120))
    assert ok and b[:4] == b"\xfc\x1d\x09\x01" and b[4:] == bytes(116)
    assert not drop.rawhex(b"1acf\n")[1]


def test_slip_types_a_bad_rd41_frame_rd94_and_fields_persist():
    from radiosonde_auto_rx_amd import drop
    good, bad3, bad2 = (synth.drop_frame(41, 7, corrupt=c) for c in ((), (0, 1, 2), (4, 5)))
    p = drop.DropPrinter(vbs=1, json=True, version="x")
    t0 = p.frame(good)
    assert p.last == (41, True) and t0.count("\n") == 3
    assert p.frame(bad3) == "" and p.last == (94, False)                  # three failing CRCs: RD94 through num_errs94 = 0, its checks fail too
    t2 = p.frame(bad2)
    assert p.last == (41, False) and t2.count("\n") == 1 and t2.endswith("# chk: 0000110\n") and "alt2" not in t2
    # a RD94 frame whose day of week is out of range keeps the weekday of the frame before
    f = bytearray(synth.drop_frame(94, 3))
    q = drop.DropPrinter()
    assert q.frame(bytes(f)).split("] ")[1].startswith("Wed")
    f[26:30] = (8 * 86400 * 1000 + 5000).to_bytes(4, "little")
    f[73:75] = synth.drop_chksum16(f[26:73]).to_bytes(2, "big")
    assert q.frame(bytes(f)).split("] ")[1].startswith("Wed")
    assert drop.DropPrinter().frame(bytes(f)).split("] ")[1].startswith("Sun")


def test_check_words_and_masks_of_generated_frames():
    from radiosonde_auto_rx_amd import drop
    for kind, blocks, full in ((41, synth.DROP_BLK41, 0x7F), (94, synth.DROP_BLK94, 0x1F)):
        f = synth.drop_frame(kind, 11)
        e94, e41 = drop.errs(f)
        assert (e41 if kind == 41 else e94) == 0
        assert bin(e94 if kind == 41 else e41).count("1") >= 3             # the other kind's checks fail: the type choice is unambiguous
        for i in range(len(blocks)):
            e = drop.errs(synth.drop_frame(kind, 11, corrupt=(i,)))
            assert (e[1] if kind == 41 else e[0]) == 1 << i
        fn, ck = (drop.crc16, synth.drop_crc16) if kind == 41 else (drop.chksum16, synth.drop_chksum16)
        for p0, n in blocks:
            assert fn(f[p0:p0 + n]) == ck(f[p0:p0 + n]) == int.from_bytes(f[p0 + n:p0 + n + 2], "big")
    assert drop.crc16(b"123456789") == 0x31C3 and drop.chksum16(bytes([1, 2, 3])) == (6 << 8 | 10)


def test_frame_from_rawbits_is_print_bitframe():
    from radiosonde_auto_rx_amd import drop
    f = synth.drop_frame(94, 5)
    raw = synth.drop_rawbits([f]).astype(np.uint8)
    d = drop.frame_from_rawbits(raw)
    assert d["bytes"] == f and d["err94"] == 0 and d["nraw"] == 2400
    cut = drop.frame_from_rawbits(raw, 1500)                                 # bits behind 1500 count as '0': 00 pairs are 'x', bytes 0
    assert cut["bytes"][:75] == f[:75] and cut["bytes"][75:] == bytes(45) and cut["nraw"] == 1500
    assert cut["err94"] == 0                                                 # blocks of zeros carry their own check word: chksum16 of zeros is 0
    raw[40:60] = 2                                                           # 'x' where a pair is neither 01 nor 10
    assert drop.frame_from_rawbits(raw)["bytes"][2] == 0
