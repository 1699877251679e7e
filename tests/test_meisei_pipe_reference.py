"""The captures tests/test_gpu_softin_meisei.py sends through the GPU modem and the Meisei consumer, through the compiled reference pipe alone, on the CPU:
`fsk_demod --cs16 -s -b -15000 -u 15000 2 48000 2400 - - | meisei100mod --softin --json --ptu --ecc` decodes every frame of both captures behind the modem's
settling time at the noise figure that module uses — so a line the device leaves out there is the device's, not the capture's."""
import re

import pytest

import test_gpu_softin_meisei as G
from golden_cases import need_ref


@pytest.mark.parametrize("variant", ["ims100", "rs11g"])
def test_reference_pipe_decodes_every_frame_of_the_captures(variant):
    if not need_ref():
        return
    assert G.NOISE == 0.05
    text = G._ref_pipe(G._capture(variant))
    # six seconds are twelve frames; the last one lacks the half symbols the modem still holds at end of input
    counters = [int(m) for m in re.findall(r"^\[(\d+)\] +\S", text, re.M)]
    assert counters == list(range(11)), text
    assert "[NO]" not in text and "(no)" not in text
    assert [int(m) for m in re.findall(r'"frame": (\d+)', text)] == [0, 2, 4, 6, 8]
    assert text.endswith("\n\n") or text.endswith(" \n")
