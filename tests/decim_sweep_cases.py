"""The rates of the decimator parity sweep (tests/test_gpu_decim_sweep.py) and what each is there to select.

One table, two readers: the GPU sweep runs every row; tests/test_decim_sweep_design.py checks, without a GPU, that the reference's
design arithmetic still gives the decimation D, tap count T, tap columns Q = ceil(T / D) and mixer-table remainder lut_len % D each
row claims — so that a row keeps aiming at the kernel variant it names when the list is edited.

IF / D / T / lut_len are the reference's own (demod_mod.c:1222-1296, `--min` = IF 32 kHz class and a transition band of IF - 12 kHz)."""

# sr, opt_min, fq (cycles per input sample), if_sr, D, T, lut_len, kernel the engine picks for it
SWEEP = [
    dict(sr=130_000,   opt_min=False, fq=0.31,    if_sr=65_000, D=2,   T=11,  lut_len=8_125,   kernel="generic Q 6, table of 8125 = odd number of samples"),
    dict(sr=250_000,   opt_min=False, fq=-0.07,   if_sr=50_000, D=5,   T=33,  lut_len=15_625,  kernel="generic"),
    dict(sr=1_024_000, opt_min=False, fq=0.0,     if_sr=51_200, D=20,  T=131, lut_len=64_000,  kernel="generic"),
    dict(sr=1_800_000, opt_min=False, fq=0.19,    if_sr=50_000, D=36,  T=239, lut_len=112_500, kernel="generic"),
    dict(sr=2_048_000, opt_min=False, fq=-0.333,  if_sr=51_200, D=40,  T=263, lut_len=128_000, kernel="generic"),
    dict(sr=2_400_000, opt_min=False, fq=0.1234,  if_sr=48_000, D=50,  T=343, lut_len=150_000, kernel="k_mix_decimate50"),
    dict(sr=2_500_000, opt_min=False, fq=0.485,   if_sr=50_000, D=50,  T=333, lut_len=156_250, kernel="k_mix_decimate50, pad 17"),
    dict(sr=2_560_000, opt_min=False, fq=-0.41,   if_sr=51_200, D=50,  T=329, lut_len=160_000, kernel="k_mix_decimate50, pad 21"),
    dict(sr=3_072_000, opt_min=False, fq=0.27,    if_sr=48_000, D=64,  T=439, lut_len=192_000, kernel="generic, D 64: 65 600 B of LDS"),
    dict(sr=3_200_000, opt_min=False, fq=-0.151,  if_sr=50_000, D=64,  T=427, lut_len=200_000, kernel="generic, D 64: 65 600 B of LDS"),
    dict(sr=3_600_000, opt_min=False, fq=0.05,    if_sr=48_000, D=75,  T=515, lut_len=225_000, kernel="wide, DS 25"),
    dict(sr=6_000_000, opt_min=False, fq=-0.22,   if_sr=48_000, D=125, T=857, lut_len=375_000, kernel="wide, DS 25"),
    dict(sr=1_600_000, opt_min=True,  fq=0.37,    if_sr=32_000, D=50,  T=319, lut_len=100_000, kernel="k_mix_decimate50, pad 31"),
    dict(sr=2_048_000, opt_min=True,  fq=-0.499,  if_sr=32_000, D=64,  T=409, lut_len=128_000, kernel="generic, D 64"),
    dict(sr=2_400_000, opt_min=True,  fq=0.0625,  if_sr=32_000, D=75,  T=479, lut_len=150_000, kernel="wide, DS 25"),
]
LONG = dict(sr=100_000, opt_min=False, fq=0.11, if_sr=50_000, D=2, T=13, lut_len=6_250, kernel="generic; IQ-DC schedule 1562 * 2^k up to 99 968 blocks")
REFUSED = dict(sr=3_216_000, opt_min=False, fq=0.0, if_sr=48_000, D=67, T=459, lut_len=201_000, kernel="none: prime D above 64, sonde_engine_create returns SONDE_E_ARG")


def case_id(c):
    return "%dk%s" % (c["sr"] // 1000, "_min" if c["opt_min"] else "")


def wide_ds(D):
    """the piece length k_mix_decimate_wide walks D in: the largest divisor of D in 4 .. 64 (sonde_engine.cpp), 0 = none"""
    for k in range(64, 3, -1):
        if D % k == 0:
            return k
    return 0
