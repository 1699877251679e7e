"""One wideband IQ stream -> every RS41, DFM, M10, M20 (and LMS6, iMet-54, Meisei, MRZ, MTS01, iMet-4 / iMet-1-RS, MkIIa, WxR-301D, RD94 / RD41 dropsondes) in it, in one process on one GPU.

The reference handles a wideband source by starting one detector process per candidate peak (auto_rx/autorx/scan.py:413-656:
rtl_power peaks -> `dft_detect` per peak) and then one decoder pipeline per sonde (decode.py).  Here the same two steps run
batched over a frequency raster: a Scanner whose channels all mix their own fq out of the shared stream (`dft_detect --IQ fq
--dc` per raster point, channel stride 0), and one demodulator Engine per detected sonde fed from the same chunks, followed by the
telemetry tier.  Everything sample-rate runs on the GPU; this module is the orchestration auto_rx does in Python.

    python -m radiosonde_auto_rx_amd.wideband --cfreq 403000000 --raster 10000 - 2400000 16 < capture.cs16

prints one JSON object per decoded frame (the reference's `rs41mod --json` object, "freq" = channel frequency in kHz).

With `--channelize` the stream goes through the polyphase channelizer first (ChannelizedReceiver, for streams of several Msps): RS41, DFM, M10,
M20, the generic family and iMet-4 are decoded from its channels; MkIIa, WxR-301D and the dropsondes are decoded by the raster receiver only.

With `--survey SECONDS` the receiver works the way auto_rx does instead of scanning a raster all the time: a spectrum survey of the stream
(power.py, the rtl_power step), auto_rx's peak pick on it, and a scanner channel per peak for the samples that follow.
"""
from __future__ import annotations

import json
import sys

import numpy as np

from .engine import Engine, snap_fq
from .scan import Scanner
from .family import DEVICE_KINDS_ALL, DEVICE_KINDS_LMS, FAMILY, LMS_BASE, FamilyDecoder
from .imet4 import Imet4Engine, Imet4Printer
from .mk2a import Mk2aEngine, Mk2aPrinter
from .wxr import WxrEngine, WxrPrinter
from .drop import DropEngine, DropPrinter
from .telemetry import DfmTelemetry, M10Telemetry, M20Telemetry, Rs41Telemetry


IMET_AFSK = ("IMET4", "IMET1RS")          # dft_detect's IMETafsk outcomes (sonde_scan.cpp): decoded by imet4.py
MK2LMS = "MK2LMS"                         # LMS6-1680 / MkIIa (scan type 18): decoded by mk2a.py
WXR = ("WXR301", "WXRPN9")                # Weathex WxR-301D, 4800 Bd / PN9 at 5000 Bd (scan types 16, 17): decoded by wxr.py
DROP = ("RD94RD41", "RD94", "RD41")       # Vaisala dropsondes (scan type 10): decoded by drop.py; the frames say which of the two it is
DROP_POOLS = ("RD94RD41", "RD94RD41 -i")  # ChannelizedReceiver: the dropsonde engine's -i is engine-wide, so a pool of slots per polarity
OWN_DEC = (MK2LMS,) + WXR + DROP          # engines with a decimation of their own: pieces are cut for them in push()


class WidebandReceiver:
    def __init__(self, sample_rate: int, *, cfreq_hz: int = 0, raster_hz: int = 10_000, span: float = 0.45, chunk: int | None = None,
                 merge_hz: float = 6_000.0, version: str = "sonde_hip", idle_s: float = 30.0, survey_s: float | None = None,
                 survey_nfft: int = 4096, dwell_s: float = 2.0, max_peaks: int = 10, snr_threshold: float = 10.0, min_distance: float = 1000.0,
                 quantization: float = 10000.0, device_family: bool = False):
        """idle_s: a decoder that has produced no frame for that long (a false detection, a sonde that has landed) is closed and its engine
        freed; the scanner starts a new one if the signal comes back.
        survey_s: None = a scanner channel on every raster point, all the time.  A number = auto_rx's cycle instead of the raster: the spectrum
        of survey_s seconds of stream (Hann, survey_nfft points, 25 % of the band edge cropped), auto_rx's peak pick on it (snr_threshold dB over
        the median, min_distance, quantization, at most max_peaks — its defaults), then a Scanner(fq=peaks, dc=True) over the next dwell_s
        seconds (what `dft_detect` per peak is to auto_rx), then the next survey.  Peaks that already have a decoder are not scanned again.
        device_family: the block codes of Meisei, iMet-54, MTS01, RS92, MRZ and LMS6 / LMS-X hits run on the device behind the frame sync (Engine.set_family) and
        decoded records come to the host instead of soft bits (LMS6: the convolutional code; Reed-Solomon and everything behind it stay with the host decoder)."""
        self.device_family = device_family
        self.sr, self.cfreq, self.merge_hz, self.version, self.idle_s = sample_rate, cfreq_hz, merge_hz, version, idle_s
        self.t = 0.0                           # stream time in seconds
        self.chunk = chunk or sample_rate // 4
        self.survey_s, self.survey = survey_s, None
        if survey_s is None:
            kmax = int(span * sample_rate / raster_hz)
            self.raster = [snap_fq(k * raster_hz / sample_rate, sample_rate) for k in range(-kmax, kmax + 1)]
            self.scanner = Scanner(sample_rate, fq=self.raster, dc=True, cont=True, max_chunk=self.chunk)
        else:
            from .power import HANN, PowerSurvey
            self.raster = [0.0]
            self.scanner = Scanner(sample_rate, fq=self.raster, dc=True, max_chunk=self.chunk)      # (only asked for its decimation factor)
            self.survey = PowerSurvey(sample_rate, survey_nfft, center_hz=float(cfreq_hz), window=HANN, crop=0.25, max_chunk=self.chunk)
            self.pick = dict(snr_threshold=snr_threshold, min_distance=min_distance, quantization=quantization, max_peaks=max_peaks)
            self.dwell_s, self._survey_t, self._scan_t0 = dwell_s, 0.0, 0.0
        # the demodulators decimate to the reference's IF rate (48 kHz, raised until it divides the sample rate, demod_mod.c:1229-1236);
        # pushes are cut at multiples of both decimation factors, the rest of a push waits for the next one
        if_sr = min(48000, sample_rate)
        while sample_rate % if_sr:
            if_sr += 1
        D = int(np.lcm(self.scanner.info["decM"], sample_rate // if_sr))
        self.align, self._rest = D, None
        self.chunk -= self.chunk % D
        self.sondes: list[dict] = []           # {fq, engine, telemetry, type, frames}
        self.log: list[dict] = []
        if self.survey is not None:            # no scanner until the first survey has named its peaks
            self.scanner.close()
            self.scanner = None

    def _survey_round(self, now: float):
        """auto_rx's scan step (scan.py:974-1137) on the spectrum gathered since the last round: pick the peaks, leave out those a decoder already
        works on, start a scanner channel on each of the others; the round's spectrum and peaks go to the log as auto_rx's scan_result has them."""
        from .power import pick_peaks
        freq, power, step = self.survey.fetch(reset=True)
        q = self.pick["quantization"]
        peaks, floor = pick_peaks(freq, power, step, min_freq=freq[0] / 1e6, max_freq=freq[-1] / 1e6, return_floor=True, **self.pick)
        lvl = [float(power[np.abs(freq - p) <= q / 2.0].max()) if (np.abs(freq - p) <= q / 2.0).any() else float(floor) for p in peaks]
        self.log.append(dict(event="survey", t=now, freq=[round(f, 6) for f in (freq / 1e6).tolist()], power=[round(v, 2) for v in power.tolist()],
                             threshold=floor, peak_freq=[p / 1e6 for p in peaks.tolist()], peak_lvl=lvl))
        active = [self.cfreq + s["fq"] * self.sr for s in self.sondes]
        todo = [p for p in peaks.tolist() if not any(abs(p - a) < q / 2.0 for a in active)]
        self._survey_t = 0.0
        if todo:
            self.raster = [snap_fq((p - self.cfreq) / self.sr, self.sr) for p in todo]
            self.scanner = Scanner(self.sr, fq=self.raster, dc=True, max_chunk=self.chunk)
            self._scan_t0 = now

    def _start(self, fq: float, typ: str, invert: bool = False):
        for s in self.sondes:
            if abs(s["fq"] - fq) * self.sr < self.merge_hz * (8 if typ in WXR else 3 if typ in ("M10", "M20") else 1):    # 9.6 kBd, and more so 64 kHz of width: seen from neighbouring raster points too
                return
        fq = snap_fq(fq, self.sr)
        khz = int(round((self.cfreq + fq * self.sr) / 1000.0)) if self.cfreq else 0
        if typ in IMET_AFSK:                                   # imet4iq --iq fq --lpIQ --dc (--imet1: 96 kHz IF), as auto_rx starts it
            eng = Imet4Engine([fq], self.sr, bits=16, iq=True, lp_iq=True, dc=True, imet1=(typ == "IMET1RS"), max_chunk=self.chunk)
            tel = Imet4Printer(json=True, jsn_freq_khz=khz, version=self.version)
        elif typ == MK2LMS:                                    # mk2a1680mod --iq fq --lpIQ --lpbw 160 --decFM --dc, as auto_rx starts it
            eng = Mk2aEngine([fq], self.sr, bits=16, opt_iq=6, lp_iq=True, lpbw_hz=160000, dec_fm=4, dc=True,
                             max_chunk=self.chunk + Mk2aEngine.dec_m_of(self.sr))     # its own IF rule (4 x 48 kHz): pieces are cut for it in push()
            tel = Mk2aPrinter(json=True, jsn_freq_khz=int((self.cfreq + fq * self.sr + 500) / 1e3) if self.cfreq > 0 else 0, show_df=True,
                              if_rate=eng.if_rate, sample_rate=self.sr, version=self.version)
        elif typ in WXR:                                       # iq_dec --FM --IFbw 64 --lpFM --iq fq | weathex301d -b --json [--pn9], as auto_rx starts it
            eng = WxrEngine([fq], self.sr, bits=16, pn9=(typ == "WXRPN9"), opt_b=True, if_bw_khz=64,
                            max_chunk=self.chunk + WxrEngine.dec_m_of(self.sr))
            tel = WxrPrinter(json=True, pn9=(typ == "WXRPN9"), jsn_freq_khz=int((self.cfreq + fq * self.sr + 500) / 1e3) if self.cfreq > 0 else 0,
                             version=self.version)
        elif typ in DROP:                                      # iq_dec --FM --lpFM --wav --bo 16 --iq fq | rd94rd41drop -b --json [-i]
            eng = DropEngine([fq], self.sr, bits=16, invert=invert, opt_b=True, max_chunk=self.chunk + DropEngine.dec_m_of(self.sr))
            tel = DropPrinter(json=True, type={"RD94": 94, "RD41": 41}.get(typ, 0),
                              jsn_freq_khz=int((self.cfreq + fq * self.sr + 500) / 1e3) if self.cfreq > 0 else 0, version=self.version)
        elif typ in FAMILY:                                    # generic sonde description + the type's bit-rate tier (family.py)
            eng = self._family_engine(typ, fq)
            tel = FamilyDecoder(typ, freq_khz=khz, version=self.version)
        elif typ == "DFM":
            eng = Engine([fq], self.sr, sonde="dfm", ecc=1, auto=True, max_chunk=self.chunk, max_frames=8)
            tel = DfmTelemetry(freq_khz=khz, version=self.version)
        elif typ in ("M10", "M20"):
            eng = Engine([fq], self.sr, sonde=typ.lower(), max_chunk=self.chunk, max_frames=8)
            tel = (M10Telemetry if typ == "M10" else M20Telemetry)(freq_khz=khz, version=self.version)
        else:
            eng = Engine([fq], self.sr, max_chunk=self.chunk, max_frames=8)
            tel = Rs41Telemetry(freq_khz=khz, version=self.version)
        self.sondes.append(dict(fq=fq, type=typ, engine=eng, telemetry=tel, frames=0, khz=khz, t_last=self.t))
        self.log.append(dict(event="detected", type=typ, fq=fq, freq_khz=khz))

    def add_channel(self, typ: str, fq: float, invert: bool = False):
        """start a decoder of sonde type `typ` (a scanner type name: "RS41", "DFM", "M10", "IMET4", "MK2LMS", "RD94RD41", ...) at fq (fraction
        of the sample rate) without waiting for the scanner — what a detection does, for signals the caller knows about or the scanner's
        48 kHz IF cannot see (an MkIIa deviates by +/- 50 kHz, a WxR-301D is 64 kHz wide).  invert: the decoder's -i (dropsondes only; a
        detection sets it from the sign of its score)."""
        self._start(fq, typ, invert)

    def _family_engine(self, typ: str, fq: float):
        f = FAMILY[typ]
        eng = Engine([fq], self.sr, sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True, lp_iq=True,
                     max_chunk=self.chunk, max_frames=8)
        eng.device_family = self.device_family and (typ in DEVICE_KINDS_ALL or typ in DEVICE_KINDS_LMS)
        if eng.device_family:
            eng.set_family(typ, ecc=FAMILY[typ]["kw"].get("ecc", 1), vit=FAMILY[typ]["kw"].get("vit", 2))
        return eng

    def _follow_lms(self, s):
        """an LMS6 whose decoder found LMS-X blocks (or the reverse): from the next chunk on its samples go through an engine of the other description
        (the stand-alone decoder replays its input from the end of the block instead, host/lms6Xmod.c; here the stream is live and that block's successor is lost)"""
        want, changed = s["telemetry"].lms_type()
        if changed and want != s["type"]:
            s["engine"].close()
            s["engine"] = self._family_engine(want, s["fq"])
            self.log.append(dict(event="retuned", type=want, was=s["type"], fq=s["fq"], freq_khz=s["khz"]))
            s["type"], s["telemetry"].moved = want, True

    def _on_detection(self, d):
        """one scanner detection -> a decoder of its type at the channel's frequency plus the offset the scanner measured"""
        if d["type"] == "RS41" and d["score"] > 0:
            self._start(self.raster[d["channel"]] + d["df"], "RS41")
        elif d["type"] == "DFM9":                                   # either polarity: the decoder runs with --auto
            self._start(self.raster[d["channel"]] + d["df"], "DFM")
        elif d["type"] in ("M10", "M20"):                           # differential code: polarity does not matter
            self._start(self.raster[d["channel"]] + d["df"], d["type"])
        elif d["type"] in IMET_AFSK:                                # the scanner's AFSK check decided the variant
            self._start(self.raster[d["channel"]] + d["df"], d["type"])
        elif d["type"] == MK2LMS:
            self.add_channel(MK2LMS, self.raster[d["channel"]] + d["df"])
        elif d["type"] in WXR:                                      # WXR301: the offset estimate is dropped, as auto_rx's scan.py does (not accurate without whitening)
            self.add_channel(d["type"], self.raster[d["channel"]] + (d["df"] if d["type"] == "WXRPN9" else 0.0))
        elif d["type"] == DROP[0]:                                  # either polarity: a negative score starts the decoder with -i
            self._start(self.raster[d["channel"]] + d["df"], DROP[0], invert=d["score"] < 0)
        elif d["type"] in FAMILY and (d["score"] > 0 or FAMILY[d["type"]]["auto"]):
            self._start(self.raster[d["channel"]] + d["df"], d["type"])

    def push(self, iq: np.ndarray, finish: bool = False):
        """iq: interleaved int16 I/Q, a whole number of chunks is not required; returns the JSON objects of this call."""
        out = []
        if self._rest is not None and len(self._rest):       # samples that did not fill a decimation block last time
            iq = np.concatenate([self._rest, np.asarray(iq, np.int16)])
        n = len(iq) // 2
        D = self.align                                        # lcm of the scanner's and the demodulators' decimation factors
        self._rest = np.array(iq[2 * (n - n % D):2 * n], np.int16)
        for s0 in range(0, n - n % D, self.chunk):
            x = iq[2 * s0:2 * min(n - n % D, s0 + self.chunk)]
            if self.scanner is not None:
                self.scanner.process_host(x, shared=True)
                for d in self.scanner.fetch():
                    self._on_detection(d)
            if self.survey is not None:
                self.survey.process_host(x)
                self._survey_t += (len(x) // 2) / self.sr
                now = self.t + (len(x) // 2) / self.sr
                if self.scanner is not None and (now - self._scan_t0 >= self.dwell_s or all(self.scanner.done(c) for c in range(len(self.raster)))):
                    self.scanner.close()
                    self.scanner = None
                if self.scanner is None and self._survey_t >= self.survey_s:
                    self._survey_round(now)
            self.t += (len(x) // 2) / self.sr
            for s in list(self.sondes):
                if s["type"] in OWN_DEC:                       # whole multiples of its decimation; the rest waits for the next piece
                    xs = np.concatenate([s["rest"], x]) if len(s.get("rest", ())) else np.asarray(x)
                    m = (len(xs) // 2) // s["engine"].dec_m * s["engine"].dec_m
                    if m:
                        s["engine"].process_host(xs[:2 * m])
                    s["rest"] = np.array(xs[2 * m:], np.int16)
                else:
                    s["engine"].process_host(x)
                before, hits = s.get("good", 0), s["frames"]
                out += self._drain(s, False)
                if s["frames"] != hits and s["type"] in ("LMS6", "LMSX"):     # any block tells what the sonde is, accepted or not
                    self._follow_lms(s)
                if s.get("good", 0) != before:      # only frames that passed their check keep a channel alive
                    s["t_last"] = self.t
                elif self.t - s["t_last"] > self.idle_s:      # silent for too long: give the engine back
                    out += self._drain(s, True)
                    s["engine"].close(); s["telemetry"].close()
                    self.sondes.remove(s)
                    self.log.append(dict(event="released", type=s["type"], fq=s["fq"], freq_khz=s["khz"], frames=s["frames"]))
        if finish:
            for s in self.sondes:
                if s["type"] in OWN_DEC:
                    s["engine"].finish()                       # the frame in progress at the end is printed as it is (mk2a1680mod.c:2409-2424, weathex301d.c:692-704, rd94rd41drop.c:1430-1445)
                out += self._drain(s, True)
        return out

    @staticmethod
    def _drain(s, finish):
        e = s["engine"]
        if s["type"] in IMET_AFSK:                           # a frame in progress at the end prints nothing (imet4iq.c:1638)
            out = []
            for f in e.fetch_frames():
                s["frames"] += 1
                js = [json.loads(line) for line in s["telemetry"].frame(f["bits"]).split("\n") if line.startswith("{")]
                s["good"] = s.get("good", 0) + (1 if js else 0)
                out += js
            return out
        if s["type"] == MK2LMS:
            out = []
            for f in e.fetch_frames():
                s["frames"] += 1
                js = [json.loads(line) for line in s["telemetry"].frame(f["bits"], f["mv"], f["df"]).split("\n") if line.startswith("{")]
                s["good"] = s.get("good", 0) + (1 if js else 0)
                out += js
            return out
        if s["type"] in WXR:                                 # -b: a frame cut short by the end of the input is printed with what it has
            out = []
            for f in e.fetch_frames():
                s["frames"] += 1
                js = [json.loads(line) for line in s["telemetry"].frame(f["bits"]).split("\n") if line.startswith("{")]
                s["good"] = s.get("good", 0) + (1 if js else 0)
                out += js
            return out
        if s["type"] in DROP:                                # JSON only for a frame with every block good; the type is what the frames say,
            out = []                                         # as auto_rx takes it from the "type" field (decode.py:1713-1717)
            for f in e.fetch_frames():
                s["frames"] += 1
                js = [json.loads(line) for line in s["telemetry"].frame(f["bytes"]).split("\n") if line.startswith("{")]
                s["good"] = s.get("good", 0) + (1 if js else 0)
                if js:
                    s["type"] = js[-1]["type"]
                out += js
            return out
        if s["type"] in FAMILY:
            out = []
            on_dev = getattr(e, "device_family", False)      # the hit's block codes ran on the device: a decoded record, not soft bits
            tel = s["telemetry"]
            # LMS6 / LMS-X: a block longer than the decoder reads (an LMS6 decoder on the LMS-X engine, the block of the change) is decoded from its soft bits
            long_lms = (lambda r: r["nbits"] > tel.lms_block_bits()) if s["type"] in DEVICE_KINDS_LMS else None
            hits = e.fetch_family(finish=finish, need_soft=long_lms) if on_dev else e.fetch_hits(finish=finish)
            for i, h in enumerate(hits):
                if on_dev and long_lms and "soft" not in h and long_lms(h):      # (the decoder changed its type on an earlier record of this very fetch)
                    h["soft"] = e.last_soft(i + 1)[i, :h["nbits"]].copy()
                s["frames"] += 1
                js = FamilyDecoder.json_objects(s["telemetry"].decoded(h, e.info["if_sr"]) if on_dev else s["telemetry"].hit(h, e.info["if_sr"]))
                s["good"] = s.get("good", 0) + (1 if js else 0)
                out += js
            return out
        frames = e.fetch_dfm(finish=finish) if s["type"] == "DFM" else e.fetch_mxx(finish=finish) if s["type"] in ("M10", "M20") else e.fetch_frames(finish=finish)
        out = []
        for fr in frames:
            js = s["telemetry"].json(fr)
            s["frames"] += 1
            s["good"] = s.get("good", 0) + int(_frame_valid(s["type"], fr))
            if js is not None:
                out.append(js)
        return out

    def close(self):
        if self.scanner is not None:
            self.scanner.close()
        if self.survey is not None:
            self.survey.close()
        for s in self.sondes:
            s["engine"].close(); s["telemetry"].close()



def _frame_valid(typ, fr):
    """a frame that passed its own check — the Reed-Solomon code (RS41), all three Hamming blocks (DFM), the checksum (M10 / M20): only such
    frames count as a sign of life when a receiver decides whether a channel has gone silent (the reference's decoders time out on the absence
    of VALID telemetry; a false detection that keeps producing garbage hits must not hold a channel)"""
    if typ == "DFM":
        return all(e >= 0 for e in fr["ecc"])
    if typ in ("M10", "M20"):
        return bool(fr["cs_ok"])
    return fr["ecc"] >= 0


class ChannelizedReceiver:
    """The same job for wide streams (BASELINE configs[2]: 10 Msps and 256 channels) without re-reading the stream once per channel:

        stream -> polyphase channelizer (chan.py: M channels at sr / D, one pass) -> Scanner on all M channels (`dft_detect --iq --dc` each)
               -> per sonde type ONE demodulator engine whose channels are handed out at run time: a detection takes a free channel
                  (sonde_engine_restart_channel), is fine-tuned to the offset the scanner measured inside its channelizer channel
                  (cfg.if_tune / sonde_engine_tune_channel) and is fed that channel's samples from then on -> telemetry JSON.

    iMet-4 goes the same way through the iMet engine (imet4.py) on the channelizer's float32 samples, `imet4iq --iq <df> --lpIQ --dc - <if_sr> 32`
    per slot: sonde_imet4_restart_channel at the scanner's offset for a detection, sonde_imet4_release_channel for a slot that has gone silent;
    released slots cost a block nothing.  An iMet-1-RS (`--imet1`: 96 kHz IF) is started only where the channelizer's output rate is at least
    96 kHz; elsewhere the log says once per sonde that it cannot be decoded at this channel rate.  The same holds for a channel rate at which
    imet4iq would decimate (an iMet-4 in a 96 kHz or 100 kHz channel: decM 2): a block's length need not be a multiple of the decimation.

    The dropsondes (RD94RD41) go through the dropsonde engine (drop.py) in its float32 form, `iq_dec --FM --lpFM --wav --bo 16 --iq <df> - <if_sr> 32 |
    rd94rd41drop -b --json [-i]` per slot: sonde_drop_restart_channel at the scanner's offset, and sonde_drop_finish_channel for a slot that has gone silent
    (with -b the frame of an open header is still printed).  The decoder's -i is engine-wide, so there are two pools of slots, one per polarity, each created
    by the first detection that needs it: a negative score takes a slot of the -i pool.  A channel rate at which iq_dec would decimate (96 kHz, 100 kHz)
    is logged once per sonde as not decodable at this channel rate.

    Not decoded here: MkIIa (+/- 50 kHz of deviation) and WxR-301D (64 kHz wide) do not fit a 50 kHz channelizer channel and are fed from the
    wide stream (WidebandReceiver).  Their detections are dropped.

    Every block costs one channelizer launch, one scanner step and one launch sequence per sonde type, whatever the number of sondes."""

    TYPES = {"RS41": ("rs41", Rs41Telemetry), "DFM": ("dfm", DfmTelemetry), "M10": ("m10", M10Telemetry), "M20": ("m20", M20Telemetry)}
    # + the scanner's RS92 / LMS6 / MEISEI / IMET5 / MRZ / MTS01: generic sonde descriptions and the bit-rate tiers of family.py
    # + IMET4 (IMET1RS at channel rates of 96 kHz and more): one Imet4Engine whose slots are restarted and released (IMET_AFSK)
    # + RD94RD41: one DropEngine per polarity whose slots are restarted, finished and released (DROP_POOLS)
    IMET1_MIN_RATE = 96000                   # --imet1's designated IF rate

    def __init__(self, sample_rate: int, *, M: int = 256, D: int = 200, P: int = 16, cfreq_hz: int = 0, slots: int = 16, chunk: int | None = None,
                 version: str = "sonde_hip", device: int = 0, idle_s: float = 30.0):
        """idle_s: a decoder channel that has produced no frame for that long (a false detection, a sonde that has landed) is ended
        (sonde_engine_finish_channel) and handed to the next detection of its type."""
        import torch
        self.idle_s, self.t = idle_s, 0.0
        self.n_if = 0                           # IF samples per channel taken so far
        from .chan import Channelizer
        from .scan import IFIQ
        self.torch, self.sr, self.cfreq, self.version, self.slots, self.device = torch, sample_rate, cfreq_hz, version, slots, device
        self.chunk = chunk or sample_rate // 4
        self.chunk -= self.chunk % D
        self.ch = Channelizer(sample_rate, M, D, P, max_chunk=self.chunk, device=device)
        self.M, self.if_sr, self.nmax = M, int(self.ch.out_rate), self.ch.max_frames
        dev = torch.device("cuda", device)
        self.out = torch.zeros(M, self.nmax, 2, dtype=torch.float32, device=dev)
        self.scanner = Scanner(self.if_sr, n_channels=M, iq_mode=IFIQ, dc=True, cont=True, max_chunk=self.nmax, device=device, bits=32)
        self.groups: dict[str, dict] = {}       # type -> {engine, stage, owner[slot] = sonde dict or None}
        self.sondes: list[dict] = []
        self.log: list[dict] = []
        self._undecodable: list[float] = []     # sondes the log has named as not decodable at this channel rate (f_hz)
        self._rest = None
        torch.cuda.synchronize(dev)

    def _group(self, typ: str):
        if typ in self.groups:                                     # (None: a type this channel rate cannot decode)
            return self.groups[typ]
        g = None
        if typ in IMET_AFSK:                        # imet4iq --iq <df> --lpIQ --dc [--imet1] - <if_sr> 32, a slot per sonde
            with self.torch.cuda.device(self.device):              # the iMet engine lives on the device that is current at create
                eng = Imet4Engine([0.0] * self.slots, self.if_sr, bits=32, iq=True, lp_iq=True, dc=True, imet1=(typ == "IMET1RS"), max_chunk=self.nmax)
            if eng.dec_m != 1:                                     # imet4iq would decimate this channel rate: blocks of any length do not fit its calls
                eng.close()
                self.groups[typ] = None
                return None
            for slot in range(self.slots):                         # handed out by restart_channel
                eng.release_channel(slot)
            stage = self.torch.zeros(self.slots, self.nmax, 2, dtype=self.torch.float32, device=self.out.device)
            self.torch.cuda.synchronize(self.out.device)
            g = self.groups[typ] = dict(engine=eng, stage=stage, owner=[None] * self.slots, calls=0)
        if typ in DROP_POOLS:                       # iq_dec --FM --lpFM --wav --bo 16 --iq <df> - <if_sr> 32 | rd94rd41drop -b --json [-i], a slot per sonde
            if DropEngine.dec_m_of(self.if_sr) != 1:               # iq_dec would decimate this channel rate: the engine's float32 form does not
                self.groups[typ] = None
                return None
            with self.torch.cuda.device(self.device):              # the engine lives on the device that is current at create
                eng = DropEngine([0.0] * self.slots, self.if_sr, bits=32, invert=(typ == DROP_POOLS[1]), opt_b=True, max_chunk=self.nmax)
            for slot in range(self.slots):                         # handed out by restart_channel
                eng.release_channel(slot)
            stage = self.torch.zeros(self.slots, self.nmax, 2, dtype=self.torch.float32, device=self.out.device)
            self.torch.cuda.synchronize(self.out.device)
            g = self.groups[typ] = dict(engine=eng, stage=stage, owner=[None] * self.slots, calls=0)
        if g is None:
            kw = dict(bits=32, iq_mode=3, if_tune=True, lp_iq=True, max_chunk=self.nmax, max_frames=8 * self.slots, device=self.device)
            if typ in FAMILY:
                f = FAMILY[typ]
                kw.update(sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True)
            else:
                kw.update(sonde=self.TYPES[typ][0])
            if typ == "DFM":
                kw.update(ecc=1, auto=True)
            eng = Engine([0.0] * self.slots, self.if_sr, **kw)
            stage = self.torch.zeros(self.slots, self.nmax, 2, dtype=self.torch.float32, device=self.out.device)
            self.torch.cuda.synchronize(self.out.device)
            g = self.groups[typ] = dict(engine=eng, stage=stage, owner=[None] * self.slots, calls=0)
        return g

    def _start(self, k: int, typ: str, df: float, invert: bool = False):
        f_hz = self.ch.channel_freq(k) + df * self.if_sr
        pool = DROP_POOLS[int(bool(invert))] if typ == DROP[0] else typ      # the engine that decodes it (self.groups)
        for s in self.sondes:                                    # the neighbouring channel sees a strong signal too
            if LMS_BASE.get(s["type"], s["type"]) == typ and abs(s["f_hz"] - f_hz) < (FAMILY[typ]["sep_hz"] if typ in FAMILY else 20_000.0 if typ in ("M10", "M20") + IMET_AFSK else 8_000.0):
                return
        # --imet1's 96 kHz IF does not fit the channel, or imet4iq decimates this channel rate (96 kHz and 100 kHz channels for an iMet-4: decM 2,
        # and a block's length need not be a multiple of it): said once per sonde
        if (typ in IMET_AFSK and ((typ == "IMET1RS" and self.if_sr < self.IMET1_MIN_RATE) or self._group(typ) is None)) or \
                (typ == DROP[0] and self._group(pool) is None):    # (a dropsonde where iq_dec decimates the channel rate)
            if not any(abs(f - f_hz) < 20_000.0 for f in self._undecodable):
                self._undecodable.append(f_hz)
                self.log.append(dict(event="not decodable at this channel rate", type=typ, f_hz=f_hz, channel=k, if_sr=self.if_sr))
            return
        g = self._group(pool)
        if None not in g["owner"]:
            self.log.append(dict(event="no free channel", type=typ, f_hz=f_hz))
            return
        slot = g["owner"].index(None)
        khz = int(round((self.cfreq + f_hz) / 1000.0)) if self.cfreq else 0
        if typ == DROP[0]:
            g["engine"].restart_channel(slot, df)                  # --iq df; the slot's sample clock starts here
            tel = DropPrinter(json=True, type=0, jsn_freq_khz=khz, version=self.version)
        elif typ in IMET_AFSK:
            g["engine"].restart_channel(slot, df)                  # --iq df: the offset inside the channelizer channel, cycles per IF sample
            tel = Imet4Printer(json=True, jsn_freq_khz=khz, version=self.version)
        else:
            if g["calls"]:
                g["engine"].restart_channel(slot)
            g["engine"].tune_channel(slot, df)
            tel = FamilyDecoder(typ, freq_khz=khz, version=self.version) if typ in FAMILY else self.TYPES[typ][1](freq_khz=khz, version=self.version)
        s = dict(type=typ, f_hz=f_hz, chan=k, slot=slot, telemetry=tel, frames=0, khz=khz, t_last=self.t, seen=0)
        g["owner"][slot] = s
        self.sondes.append(s)
        if typ == DROP[0]:
            s["invert"] = bool(invert)
        self.log.append(dict(event="detected", type=typ, f_hz=f_hz, channel=k, slot=slot, freq_khz=khz, if_sample=self.n_if, **({"invert": bool(invert)} if typ == DROP[0] else {})))   # if_sample: the slot's first sample, counted in the channel's IF samples from the start of the stream

    def add_channel(self, typ: str, f_hz: float, invert: bool = False):
        """start a decoder of sonde type `typ` (a scanner type name the receiver decodes: "RS41", "DFM", "M10", "IMET4", "LMS6", "RD94RD41", ...) at
        f_hz (Hz from the stream's centre) without waiting for the scanner, from the next block on — what a detection does: the nearest channelizer
        channel and the offset that is left inside it.  invert: the decoder's -i (dropsondes only; a detection sets it from the sign of its score)."""
        if typ not in self.TYPES and typ not in FAMILY and typ not in IMET_AFSK and typ != DROP[0]:
            raise ValueError("the channelized receiver has no decoder for %r" % (typ,))
        k = self.ch.nearest_channel(f_hz)
        self._start(k, typ, (f_hz - self.ch.channel_freq(k)) / self.if_sr, invert and typ == DROP[0])

    def _on_detection(self, d):
        """one scanner detection -> a decoder slot of its type at the offset the scanner measured inside the channel"""
        if d["type"] == "RS41" and d["score"] > 0:
            self._start(d["channel"], "RS41", d["df"])
        elif d["type"] == "DFM9":
            self._start(d["channel"], "DFM", d["df"])
        elif d["type"] in ("M10", "M20"):
            self._start(d["channel"], d["type"], d["df"])
        elif d["type"] in IMET_AFSK:                               # the scanner's AFSK check decided the variant
            self._start(d["channel"], d["type"], d["df"])
        elif d["type"] == DROP[0]:                                 # either polarity: a negative score takes a slot of the -i pool
            self._start(d["channel"], DROP[0], d["df"], invert=d["score"] < 0)
        elif d["type"] in FAMILY and (d["score"] > 0 or FAMILY[d["type"]]["auto"]):
            self._start(d["channel"], d["type"], d["df"])

    def push(self, iq: np.ndarray, finish: bool = False):
        """iq: interleaved int16 I/Q of the wide stream; returns the JSON objects of this call."""
        torch = self.torch
        out = []
        if self._rest is not None and len(self._rest):
            iq = np.concatenate([self._rest, np.asarray(iq, np.int16)])
        n = len(iq) // 2
        D = self.sr // self.if_sr
        self._rest = np.array(iq[2 * (n - n % D):2 * n], np.int16)
        for s0 in range(0, n - n % D, self.chunk):
            x = np.ascontiguousarray(iq[2 * s0:2 * min(n - n % D, s0 + self.chunk)])
            m = self.ch.process_host(x, self.out.data_ptr(), self.nmax)           # m IF samples per channel
            self.ch.sync()
            self.scanner.process_device(self.out.data_ptr(), self.nmax, m)
            for d in self.scanner.fetch():
                self._on_detection(d)
            for typ, g in list(self.groups.items()):
                if g is None:                                                     # a type this channel rate cannot decode (_group)
                    continue
                for slot, s in enumerate(g["owner"]):
                    if s is not None:
                        g["stage"][slot, :m] = self.out[s["chan"], :m]
                torch.cuda.synchronize(self.out.device)                           # the copies ran on torch's stream, the engine has its own
                if typ in IMET_AFSK or typ in DROP_POOLS:
                    g["engine"].process_device(g["stage"].data_ptr(), m, ch_stride=self.nmax)
                else:
                    g["engine"].process_device(g["stage"].data_ptr(), self.nmax, m)
                g["calls"] += 1
                out += self._drain(typ, g, False)
                for slot, s in enumerate(g["owner"]):                             # channels that have gone silent go back to the pool
                    if s is None:
                        continue
                    if s.get("good", 0) != s["seen"]:                              # only frames that passed their check keep a channel
                        s["seen"], s["t_last"] = s.get("good", 0), self.t
                    elif self.t - s["t_last"] > self.idle_s:
                        if typ in IMET_AFSK:                                       # the frame in progress prints nothing (imet4iq.c:1638)
                            g["engine"].release_channel(slot)
                        else:
                            g["engine"].finish_channel(slot)
                            out += self._drain(typ, g, False)                     # what the end of its stream still gave
                        g["owner"][slot] = None
                        s["telemetry"].close()
                        self.sondes.remove(s)
                        self.log.append(dict(event="released", type=DROP[0] if typ in DROP_POOLS else typ, f_hz=s["f_hz"], slot=slot, frames=s["frames"]))
            for s in [s for s in self.sondes if s["type"] in ("LMS6", "LMSX")]:     # after every engine has had this block: sondes whose decoder changed type
                self._follow_lms(s)
            self.t += m / self.if_sr
            self.n_if += m
        if finish:
            for typ, g in self.groups.items():
                if g is None:
                    continue
                if typ in DROP_POOLS:                                             # the frame in progress at the end is printed as it is (rd94rd41drop.c:1430-1445)
                    for slot, s in enumerate(g["owner"]):
                        if s is not None:
                            g["engine"].finish_channel(slot)
                out += self._drain(typ, g, True)
        return out

    def _follow_lms(self, s):
        """an LMS6 whose decoder found LMS-X blocks (or the reverse): the sonde moves to a channel of the engine of the other description, decoder object and
        all; the next block of samples is the first it sees there"""
        want, changed = s["telemetry"].lms_type()
        if not changed or want == s["type"]:
            return
        g0 = self.groups[s["type"]]
        g0["engine"].finish_channel(s["slot"])
        g0["owner"][s["slot"]] = None
        g = self._group(want)
        if None not in g["owner"]:
            s["telemetry"].close()
            self.sondes.remove(s)
            self.log.append(dict(event="no free channel", type=want, f_hz=s["f_hz"]))
            return
        slot = g["owner"].index(None)
        if g["calls"]:
            g["engine"].restart_channel(slot)
        g["engine"].tune_channel(slot, (s["f_hz"] - self.ch.channel_freq(s["chan"])) / self.if_sr)
        self.log.append(dict(event="retuned", type=want, was=s["type"], f_hz=s["f_hz"], slot=slot))
        s["type"], s["slot"], s["telemetry"].moved = want, slot, True
        g["owner"][slot] = s

    def _drain(self, typ, g, finish):
        e = g["engine"]
        if typ in IMET_AFSK:                                       # as WidebandReceiver._drain: a frame is a sign of life when it printed a JSON object
            out = []
            for f in e.fetch_frames():
                s = g["owner"][f["channel"]]
                if s is None:
                    continue
                s["frames"] += 1
                js = [json.loads(line) for line in s["telemetry"].frame(f["bits"]).split("\n") if line.startswith("{")]
                s["good"] = s.get("good", 0) + (1 if js else 0)
                out += js
            return out
        if typ in DROP_POOLS:                                      # JSON only for a frame with every block good; its "type" says which of the two it is
            out = []
            for f in e.fetch_frames():
                s = g["owner"][f["channel"]]
                if s is None:
                    continue
                s["frames"] += 1
                js = [json.loads(line) for line in s["telemetry"].frame(f["bytes"]).split("\n") if line.startswith("{")]
                s["good"] = s.get("good", 0) + (1 if js else 0)
                out += js
            return out
        if typ in FAMILY:                                          # header hits -> the type's bit-rate tier (family.py), one decoder object per sonde
            out = []
            for h in e.fetch_hits(finish=finish):
                s = g["owner"][h["channel"]]
                if s is None:
                    continue
                s["frames"] += 1
                js = FamilyDecoder.json_objects(s["telemetry"].hit(h, self.if_sr))
                s["good"] = s.get("good", 0) + (1 if js else 0)
                out += js
            return out
        frames = e.fetch_dfm(finish=finish) if typ == "DFM" else e.fetch_mxx(finish=finish) if typ in ("M10", "M20") else e.fetch_frames(finish=finish)
        out = []
        for fr in frames:
            s = g["owner"][fr["channel"]]
            if s is None:
                continue
            js = s["telemetry"].json(fr)
            s["frames"] += 1
            s["good"] = s.get("good", 0) + int(_frame_valid(typ, fr))
            if js is not None:
                out.append(js)
        return out

    def close(self):
        self.scanner.close(); self.ch.close()
        for g in self.groups.values():
            if g is not None:
                g["engine"].close()
        for s in self.sondes:
            s["telemetry"].close()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfreq", type=int, default=0, help="centre frequency of the stream in Hz (for the JSON freq field)")
    ap.add_argument("--raster", type=int, default=10_000, help="scanner raster in Hz")
    ap.add_argument("--survey", type=float, default=None, metavar="SECONDS", help="auto_rx's cycle instead of the raster: a spectrum survey of that many seconds, peak pick, a scanner channel per peak")
    ap.add_argument("--channelize", action="store_true", help="polyphase channelizer front end (256 channels at sr / 200): for streams of several Msps")
    ap.add_argument("--device-family", action="store_true", help="decode Meisei, iMet-54, MTS01, RS92, MRZ and LMS6 / LMS-X hits on the device (not with --channelize)")
    ap.add_argument("--rs92-ephem", help="RINEX navigation file for RS92 positions (rs92mod -e)")
    ap.add_argument("--rs92-alm", help="SEM almanac for RS92 positions (rs92mod -a)")
    ap.add_argument("dash"); ap.add_argument("sr", type=int); ap.add_argument("bits", type=int)
    a = ap.parse_args(argv)
    if a.rs92_ephem or a.rs92_alm:
        from .family import set_rs92_orbits
        set_rs92_orbits(ephemeris=a.rs92_ephem, almanac=a.rs92_alm)
    if a.dash != "-" or a.bits != 16:
        ap.error("input is `- <sr> 16` (cs16 on stdin)")
    if a.channelize and a.survey is not None:
        ap.error("--survey belongs to the raster receiver (the channelized one scans all its channels)")
    rx = ChannelizedReceiver(a.sr, cfreq_hz=a.cfreq) if a.channelize else WidebandReceiver(a.sr, cfreq_hz=a.cfreq, raster_hz=a.raster, survey_s=a.survey, device_family=a.device_family)
    inp = sys.stdin.buffer
    while True:
        buf = inp.read(rx.chunk * 4)
        last = len(buf) < rx.chunk * 4                        # also an EMPTY read: the frame in progress at EOF is still due
        for js in rx.push(np.frombuffer(buf[:len(buf) // 4 * 4], np.int16), finish=last):
            print(json.dumps(js), flush=True)
        if last:
            break
    rx.close()


if __name__ == "__main__":
    main()
