"""The iMet printer's lines through auto_rx's own line handler (SondeDecoder.handle_decoder_line, sonde type "IMET"), in the way
tests/test_caller_contract.py does it for the other decoders: the frames the reference decoded, printed here, give auto_rx the same
telemetry as the reference's own stdout for that capture.  Skips where the auto_rx sources are absent."""
import os
import sys
import types

import pytest

from tests import imet4_cases as cases

AUTORX = "/root/reference/auto_rx"
pytestmark = pytest.mark.skipif(not os.path.isdir(AUTORX), reason="needs the auto_rx sources")


@pytest.fixture(scope="module")
def autorx():
    sys.modules.setdefault("semver", types.ModuleType("semver"))
    if AUTORX not in sys.path:
        sys.path.insert(0, AUTORX)
    import autorx as pkg
    import autorx.decode
    return pkg


def _telemetry(autorx, stdout: bytes):
    d = object.__new__(autorx.decode.SondeDecoder)
    sink, rets = [], []
    d.raw_file = None; d.udp_mode = False; d.sonde_type = "IMET"; d.sonde_freq = 402.5e6; d.rx_frequency = 402.5e6
    d.sdr_type = "RTLSDR"; d.rtl_device_idx = "0"; d.sdr_hostname = "localhost"; d.sdr_port = 5555
    d.close_on_encrypted = False; d.exporters = [sink.append]; d.demod_stats = None
    d.telem_filter = None; d.enable_realtime_filter = False; d.last_positions = {}; d.max_velocity = 1000
    d.rs41_subframe_uploads = []; d.imet_type = None; d.imet_prev_frame = None; d.imet_prev_time = None; d.imet_id = []; d.imet_max_ids = 4
    d.exit_state = "OK"; d.decoder_running = True
    for line in stdout.split(b"\n"):
        if line:
            rets.append(d.handle_decoder_line(line + b"\n"))
    return sink, rets


def test_auto_rx_reads_our_imet_lines_like_the_references(autorx):
    from tests.test_imet4_fields import _frames, _print
    g = cases.load("48k_off1500")
    frames = _frames(g["stdout"][g["argv"].index(cases.IMET + ["--rawbits"])])
    ver = autorx.__version__
    for argv, ref in zip(g["argv"][:2], g["stdout"][:2]):
        ours = _print(frames, json=True, version=ver, **({"jsn_freq_khz": 402500} if "--jsn_cfq" in argv else {}))
        theirs = ref.replace(b'"version": "oracle"', ('"version": "%s"' % ver).encode())
        a, ra = _telemetry(autorx, ours)
        b, rb = _telemetry(autorx, theirs)
        assert len(a) == len(b) >= 4 and ra == rb          # (auto_rx holds back the first frame of an iMet while it forms its ID)
        for x, y in zip(a, b):
            x, y = dict(x), dict(y)
            for k in ("time_received",):
                x.pop(k, None); y.pop(k, None)
            assert x == y
        assert a[0]["type"].startswith("IMET") and a[0]["lat"] == pytest.approx(39.76553)
