"""Life cycle of every kind of host object behind the C ABI: create, one process call, fetch, destroy — three times in a row in one process.
Every return code is 0 (the bindings raise otherwise) and the third instance's fetched output equals the first's byte for byte: a new
object starts from fresh state whatever its predecessors left on the device, and destroying one takes nothing of the next with it.  Each case
enters the allocations its kind makes on first use (the 8-bit copy, the restart buffers, the channelizer's own output and rows, the staging
buffers of the process_host calls) once before the destroy.

Then the configurations that are refused only after a create has begun to allocate: the return codes are those of the revision before
the host objects got their owner (SONDE_E_ARG each, taken from a run of these calls against that build), and a valid create of the same
kind works right behind the refusal.

One call of at most 0.1 s of input per instance.  Nothing here looks at the device's free memory (the card is shared); that nothing leaks
is the business of tests/test_devmem.py and of the structure (one owner per object, destroy = delete)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR, N = 2_400_000, 240_000            # the 2.4 Msps engines: 0.1 s a call
E_ARG = -1


def _noise(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(96, 160, shape).astype(np.uint8)
    if dtype == np.float32:
        return (0.05 * rng.standard_normal(shape)).astype(np.float32)
    return rng.integers(-2000, 2000, shape).astype(np.int16)


X16 = _noise((3, 2 * N), np.int16, 1)           # shared by the cases, never written


def _raw(pair):
    buf, n = pair
    return bytes(buf)[:n * C.sizeof(buf._type_)]


def _engine(x, fetch=lambda e: e.fetch_frames_np().tobytes(), before=None, sample_rate=SR, max_chunk=N, **kw):
    def run():
        from radiosonde_auto_rx_amd.engine import Engine
        eng = Engine([0.1], sample_rate, max_chunk=max_chunk, **kw)
        if before:
            before(eng)
        eng.process_host(x)
        eng.sync()
        out = fetch(eng) + eng.sync_state().tobytes()
        eng.close()
        return out
    return run


def _mixed():
    import torch
    from radiosonde_auto_rx_amd.engine import MixedEngine
    eng = MixedEngine([0.1, -0.12, 0.2], ["rs41", "dfm", "m10"], SR, max_chunk=N)
    summ = torch.zeros(3, 32, dtype=torch.uint8, device="cuda")      # one sonde_summary_t per channel, written by every group's frame sync
    torch.cuda.synchronize()
    eng.set_summary(summ.data_ptr())
    eng.process_host(X16)
    eng.sync()
    out = eng.fetch_frames_np().tobytes() + _raw(eng.fetch_dfm_raw()) + _raw(eng.fetch_m10_raw())
    out += summ.cpu().numpy().tobytes() + repr([eng.group_info(c) for c in range(3)]).encode()
    eng.close()
    return out


def _scanner(**kw):
    from radiosonde_auto_rx_amd.scan import Scanner
    sc = Scanner(SR, fq=[0.1], max_chunk=N, **kw)
    sc.process_host(X16[:1])
    out = repr(sc.fetch()).encode() + repr(sc.info).encode()
    sc.close()
    return out


def _fsk():
    from radiosonde_auto_rx_amd.fsk import FskModem
    md = FskModem(48_000, 4800, n_channels=1, P=5, max_chunk=4800)
    md.process_host(X16[:1, :2 * 4800])
    sd, recs = md.fetch(0)
    md.close()
    return sd.tobytes() + repr(recs).encode()


def _chan():
    import torch
    from radiosonde_auto_rx_amd.chan import Channelizer
    ch = Channelizer(1_200_000, 64, 50, 8, max_chunk=120_000)
    own, stride = ch.output()
    rows = ch.rows_alloc(2)
    assert own and rows and stride == ch.max_frames
    out = torch.zeros(64, ch.max_frames, 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                     # the fill runs on torch's stream, the channelizer on its own: order them
    k = ch.process_host(X16[0, :2 * 120_000], out.data_ptr(), ch.max_frames)
    k2 = ch.process_host(X16[1, :2 * 100], own, stride)             # a call shorter than the filter's history: the staging buffer
    ch.gather(own, stride, [3, -1], k2, rows)
    ch.sync()
    res = out.cpu().numpy()[:, :k].tobytes() + repr((k, k2)).encode()
    ch.close()
    return res


def _power():
    from radiosonde_auto_rx_amd.power import PowerSurvey
    ps = PowerSurvey(SR, 4096, max_chunk=N)
    ps.process_host(X16[0])
    out = ps.fetch()[1].tobytes() + repr(ps.segments()).encode()
    ps.close()
    return out


def _softin_m10():
    from radiosonde_auto_rx_amd.fsk import FskModem, SoftinDev
    md = FskModem(48_080, 9616, n_channels=1, P=5, nsym=50, lower=-10000, upper=10000, max_chunk=4808)
    sf = SoftinDev(1, kind="m10", ecc=0, inv=False)
    md.process_host(X16[:1, :2 * 4808])
    sf.push_fsk(md)
    out = repr(sf.fetch_m10()).encode() + repr(sf.counts()).encode()
    sf.close(); md.close()
    return out


def _imet4():
    from radiosonde_auto_rx_amd.imet4 import Imet4Engine
    eng = Imet4Engine([0.0], 48_000, max_chunk=4800)
    eng.process_host(X16[:1, :2 * 4800])
    out = repr(eng.fetch_frames()).encode() + repr(eng.read_state(0)).encode()
    eng.close()
    return out


CASES = {
    "rs41_s16": _engine(X16[:1]),
    "m10": _engine(X16[:1], fetch=lambda e: _raw(e.fetch_m10_raw()), sonde="m10", ecc=0),
    "rs41_dc": _engine(X16[:1], opt_dc=True),
    "rs41_cf32": _engine(_noise((1, 2 * N), np.float32, 2), bits=32),
    "rs41_u8": _engine(_noise((1, 2 * N), np.uint8, 3), bits=8),
    "rs41_audio": _engine(X16[:1, :4800], audio=True, sample_rate=48_000, max_chunk=4800),
    "rs41_restarted": _engine(X16[:1], before=lambda e: e.restart_channel(0)),
    "mixed_rs41_dfm_m10": _mixed,
    "scanner_bbiq": _scanner,
    "fsk_modem": _fsk,
    "channelizer": _chan,
    "power": _power,
    "softin_m10": _softin_m10,
    "imet4": _imet4,
}


@pytest.mark.parametrize("name", list(CASES))
def test_three_instances_in_a_row(name):
    outs = [CASES[name]() for _ in range(3)]
    assert len(outs[0]) > 0
    assert outs[2] == outs[0]


# ---- refused behind the first allocations --------------------------------------------------------------------------------------------

def _code(exc) -> int:
    """the SONDE_E_* code of a SondeError raised by a binding"""
    import re
    m = re.search(r"\((-\d+)\)", str(exc)) or re.search(r"(-\d+)", str(exc))
    return int(m.group(1))


def _mixed_create(group_of_channel, n_groups):
    from radiosonde_auto_rx_amd.engine import ABI_VERSION, LP_IQ, SONDE_MIXED, SONDE_RS41, SondeCfg, SondeGroup, lib
    n_ch = len(group_of_channel)
    cfg = SondeCfg(ABI_VERSION, 0, n_ch, SR, 16, SONDE_MIXED, LP_IQ, 0, 0, 0, 0, 0.0, N, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0)
    groups = (SondeGroup * n_groups)(*[SondeGroup(SONDE_RS41, 2, 0, 0, 0, 0, 0.0, 0) for _ in range(n_groups)])
    fq = np.linspace(-0.2, 0.2, n_ch)
    gof = np.asarray(group_of_channel, dtype=np.int32)
    h = C.c_void_p()
    rc = lib().sonde_engine_create_mixed(C.byref(cfg), fq.ctypes.data_as(C.POINTER(C.c_double)), groups, n_groups, gof.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h))
    if rc == 0:
        lib().sonde_engine_destroy(h)
    return rc


def test_rejections_behind_allocations_keep_their_codes():
    from radiosonde_auto_rx_amd.engine import Engine, SondeError
    from radiosonde_auto_rx_amd.scan import Scanner
    # pipeline with FM audio input (once refused where stream B was made, behind every buffer of the engine)
    with pytest.raises(SondeError) as e:
        Engine([0.0], 48_000, audio=True, pipeline=True, max_chunk=4800)
    assert _code(e.value) == E_ARG
    assert len(CASES["rs41_audio"]()) > 0
    # a channel whose group does not exist; more groups than a mixed engine takes
    assert _mixed_create([0, 1, 2], 2) == E_ARG
    assert _mixed_create([0, 1, -1], 2) == E_ARG
    assert _mixed_create([0, 1, 2], 65) == E_ARG
    assert _mixed_create([0, 1, 1], 2) == 0
    assert len(_mixed()) > 0
    # a scanner whose windows would need a transform beyond 32768 points (IF rate 600 kHz): refused behind the front end's tables
    with pytest.raises(SondeError) as e:
        Scanner(SR, fq=[0.1], max_chunk=N, bw_khz=600.0)
    assert _code(e.value) == E_ARG
    assert len(_scanner()) > 0
