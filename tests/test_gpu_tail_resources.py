"""Workgroups per compute unit of the IF-rate tail, asked of the runtime for the kernels and the dynamic LDS an engine really launches with
(sonde_engine_tail_residency -> hipOccupancyMaxActiveBlocksPerMultiprocessor).  The headline engine's IF chain keeps (X1, X2) in storage that is
dead by then and must hold at least seven workgroups per CU (six before: 23.9 KB of LDS each); its k_search_sync must hold exactly two, so that 512
channels stay one wave of workgroups on 256 CUs.  A --dc engine (discriminator and 97-tap FM low-pass: 39.4 KB and four workgroups before, 20.3 KB
now) must hold at least six."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR = 2_400_000


def _fqs(n):
    from tools import synth
    return [synth.snap_fq(-0.4 + 0.8 * i / n, SR) for i in range(n)]


def test_headline_engine_residency():
    from radiosonde_auto_rx_amd.engine import Engine
    eng = Engine(_fqs(512), SR, lp_iq=True, ecc=2, max_chunk=SR, max_frames=2048)
    r = eng.tail_residency()
    eng.close()
    print("headline residency", r)
    assert r["if_chain"] >= 7, r
    assert r["search_sync"] == 2, r


def test_dc_engine_residency():
    from radiosonde_auto_rx_amd.engine import Engine
    eng = Engine(_fqs(8), SR, lp_iq=True, ecc=2, opt_dc=True, max_chunk=SR, max_frames=64)
    r = eng.tail_residency()
    eng.close()
    print("--dc residency", r)
    assert r["if_chain"] >= 6, r
    assert r["search_sync"] == 0, r          # --dc engines correlate in the time domain and run k_framesync
