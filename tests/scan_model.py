"""The station finder (fmd_scan_*, csrc/scan.inc) in float64: the definition of include/fmdemod_mi355x.h, "Station finder", step by step and in the
same order of additions - A from zero over the blocks, Pc and M from zero over the bins s0 .. s1 upwards, one rounded product per term - so its
doubles are the device's where the device keeps to the definition.  Also here: the plan in Python integers, the decision margins of a case, the
comparison a device result is held to (assert_matches: the tolerances of the definition's floats), planted defects, the fixed case list of
tests/test_scan_cpu.py and tests/test_gpu_scan.py, and the synthetic capture of the end-to-end test."""
import numpy as np

E_ARG, E_UNSUPPORTED = -1, -2
MAX_BINS, MAX_CANDIDATES, MAX_STATIONS = 4096, 1024, 64

STATION_DTYPE = np.dtype([("offset_hz", "<i4"), ("candidate", "<i4"), ("power", "<f4"), ("snr", "<f4"), ("centroid_hz", "<f4"), ("reserved", "<i4", (3,))])

DEFECTS = ("bins_off_by_one", "guard_ignored", "tie_reversed", "window_short", "floor_over_all", "nyquist_counted")


class Refused(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status


def config(rate, n_bins, raster_hz, bw, min_sep=1, floor_permille=250, dc_guard=0, max_stations=16, threshold=4.0, reserved=(0, 0, 0)):
    return dict(rate=rate, n_bins=n_bins, raster_hz=raster_hz, bw=bw, min_sep=min_sep, floor_permille=floor_permille, dc_guard=dc_guard,
                max_stations=max_stations, threshold=threshold, reserved=tuple(reserved))


def plan(cfg, defect=None):
    """the range check and the plan in Python integers: dict(C, cmax, rank, n_used, nb, first, count, w_first, w_last); Refused outside the range"""
    R, N, ras, bw = cfg["rate"], cfg["n_bins"], cfg["raster_hz"], cfg["bw"]
    thr = np.float32(cfg["threshold"])
    if any(cfg["reserved"]):
        raise Refused(E_ARG, "reserved")
    if R <= 0:
        raise Refused(E_ARG, "rate")
    if N < 64 or N > MAX_BINS or N & (N - 1):
        raise Refused(E_UNSUPPORTED, "n_bins")
    if ras <= 0:
        raise Refused(E_ARG, "raster_hz")
    if bw <= 0 or R > 2 * bw * N:
        raise Refused(E_ARG, "bw")
    room = (R - 2 * bw) * N - (0 if defect == "nyquist_counted" else R)
    if room < 0:
        raise Refused(E_ARG, "cmax")
    cmax = room // (2 * N * ras)
    C = 2 * cmax + 1
    if C > MAX_CANDIDATES:
        raise Refused(E_UNSUPPORTED, "C")
    if not 1 <= cfg["min_sep"] <= C:
        raise Refused(E_ARG, "min_sep")
    if not 0 <= cfg["floor_permille"] <= 1000:
        raise Refused(E_ARG, "floor_permille")
    if not 0 <= cfg["dc_guard"] <= N // 4:
        raise Refused(E_ARG, "dc_guard")
    if not 1 <= cfg["max_stations"] <= MAX_STATIONS:
        raise Refused(E_ARG, "max_stations")
    if not np.isfinite(thr) or not thr > 0:
        raise Refused(E_ARG, "threshold")
    g = cfg["dc_guard"]
    n_used = N if defect == "floor_over_all" else N - max(0, 2 * g - 1)
    first, count, w_first, w_last = [], [], [], []
    for i in range(C):
        ctr = (i - cmax) * ras
        lo2, hi2 = 2 * N * (ctr - bw), 2 * N * (ctr + bw)          # in units of 1 / (2 N) Hz: bin s covers [(2 s - 1) R, (2 s + 1) R)
        s0 = (lo2 + R) // (2 * R)
        s1 = -((-(hi2 + R)) // (2 * R)) - 1
        first.append(s0 + (1 if defect == "bins_off_by_one" else 0))
        count.append(s1 - s0 + 1)
        w_first.append(float((2 * s0 + 1) * R - lo2) / float(2 * R))
        w_last.append(float(hi2 - (2 * s1 - 1) * R) / float(2 * R))
    return dict(C=C, cmax=cmax, rank=(cfg["floor_permille"] * (n_used - 1)) // 1000, n_used=n_used, nb=float(2 * bw * N) / float(R),
                first=first, count=count, w_first=w_first, w_last=w_last)


def scan_stream(P, cfg, defect=None):
    """one stream: P float32 [n_blocks, n_bins] -> dict of the doubles (A, F, Fc, lim, Pc, M), the decisions (occupied, station, order) and the
    fields of the ranked stations as the definition rounds them"""
    P = np.asarray(P, dtype=np.float32)
    n_blocks, N = P.shape
    assert N == cfg["n_bins"] and n_blocks >= 1
    pl = plan(cfg, defect)
    C, cmax = pl["C"], pl["cmax"]
    acc = np.zeros(N, np.float64)
    for b in range(n_blocks):
        acc = acc + P[b].astype(np.float64)
    A = acc / np.float64(n_blocks)
    k = np.arange(N)
    s_abs = np.where(k < N // 2, k, N - k)
    g = 0 if defect == "guard_ignored" else cfg["dc_guard"]
    guarded = s_abs < g
    used = np.ones(N, bool) if defect == "floor_over_all" else ~guarded
    F = np.sort(A[used])[pl["rank"] if defect != "guard_ignored" else (cfg["floor_permille"] * (N - 1)) // 1000]
    A = np.where(guarded, F, A)
    Pc, M = np.zeros(C), np.zeros(C)
    for i in range(C):
        s = pl["first"][i] + np.arange(pl["count"][i])
        term = A[s & (N - 1)].copy()
        term[0] = pl["w_first"][i] * term[0]
        if term.size > 1:
            term[-1] = pl["w_last"][i] * term[-1]
        d = (s * cfg["rate"] - (i - cmax) * cfg["raster_hz"] * N).astype(np.float64) * (1.0 / N)
        Pc[i] = np.cumsum(term)[-1]
        M[i] = np.cumsum(term * d)[-1]
    Fc = F * pl["nb"]
    lim = np.float64(np.float32(cfg["threshold"])) * Fc
    occupied = Pc > lim
    sep = cfg["min_sep"] - (1 if defect == "window_short" else 0)

    def beats(j, i):
        if Pc[j] != Pc[i]:
            return Pc[j] > Pc[i]
        return j > i if defect == "tie_reversed" else j < i

    station = np.zeros(C, bool)
    for i in np.nonzero(occupied)[0]:
        station[i] = not any(beats(j, i) for j in range(max(0, i - sep), min(C - 1, i + sep) + 1) if j != i)
    idx = [int(i) for i in np.nonzero(station)[0]]
    order = sorted(idx, key=lambda i: (-Pc[i], i if defect != "tie_reversed" else -i))
    found, written = len(order), min(len(order), cfg["max_stations"])
    st = np.zeros(cfg["max_stations"], STATION_DTYPE)
    centroid = np.zeros(written)
    with np.errstate(divide="ignore", invalid="ignore"):
        for r, i in enumerate(order[:written]):
            off = (i - cmax) * cfg["raster_hz"]
            centroid[r] = off + M[i] / Pc[i]
            st[r] = (off, i, np.float32(Pc[i]), np.float32(Pc[i] / Fc), np.float32(centroid[r]), (0, 0, 0))
    return dict(plan=pl, A=A, F=F, Fc=Fc, lim=lim, Pc=Pc, M=M, occupied=occupied, station=station, order=order, found=found, written=written,
                stations=st, centroid=centroid, chan=Pc.astype(np.float32))


def scan(power, cfg, defect=None):
    """power float32 [n_streams, n_blocks, n_bins] -> one scan_stream result per stream"""
    return [scan_stream(p, cfg, defect) for p in np.asarray(power, dtype=np.float32)]


def margins(res, cfg):
    """(occupancy margin, order margin, exact ties) of one stream's result: the smallest |Pc / (threshold Fc) - 1| over the candidates, the smallest
    |Pc[i] / Pc[j] - 1| over the pairs a decision compares - an occupied i with every j within min_sep, and neighbours in the ranked list - leaving
    out the pairs that are EXACTLY equal, which are counted instead (a deliberate tie is decided by the index, on any arithmetic).  With lim = 0 the
    occupancy decision is Pc > 0, exact on any arithmetic (a sum of non-negative terms is zero only when all are): margin inf."""
    Pc, lim = res["Pc"], res["lim"]
    with np.errstate(divide="ignore", invalid="ignore"):
        occ = float(np.min(np.abs(Pc / lim - 1.0))) if lim > 0 else np.inf
    best, ties = np.inf, 0
    pairs = set()
    C = Pc.size
    for i in np.nonzero(res["occupied"])[0]:
        for j in range(max(0, i - cfg["min_sep"]), min(C - 1, i + cfg["min_sep"]) + 1):
            if j != i:
                pairs.add((min(i, j), max(i, j)))
    for a, b in zip(res["order"][:-1], res["order"][1:]):
        pairs.add((min(a, b), max(a, b)))
    for i, j in pairs:
        if Pc[i] == Pc[j]:
            ties += 1
        elif Pc[i] > 0 and Pc[j] > 0:                    # (against an exact zero the comparison is exact on any arithmetic)
            best = min(best, abs(Pc[i] / Pc[j] - 1.0))
    return occ, best, ties


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32)))


def assert_matches(res, stations, counts, chan, cfg, what=""):
    """a device result of one stream (stations STATION_DTYPE [max_stations], counts int32 [2], chan float32 [C] or None) against the model's: found,
    written, candidate and offset_hz equal; power, snr and chan within one float32 ulp of the model's rounded value; centroid_hz within
    2^-23 max(|centroid_hz|, bw) of the model's double; the slots beyond `written` all-zero bytes"""
    stations = np.asarray(stations).view(STATION_DTYPE).reshape(-1)
    assert stations.size == cfg["max_stations"], what
    assert (int(counts[0]), int(counts[1])) == (res["found"], res["written"]), (what, counts, res["found"], res["written"])
    w = res["written"]
    want = res["stations"]
    assert np.array_equal(stations["candidate"][:w], want["candidate"][:w]), (what, stations["candidate"][:w], want["candidate"][:w])
    assert np.array_equal(stations["offset_hz"][:w], want["offset_hz"][:w]), what
    assert not np.asarray(stations[:w]["reserved"]).any(), what
    assert not stations[w:].tobytes().strip(b"\0"), (what, "slots beyond written are not zero")
    for f in ("power", "snr"):
        g, m = stations[f][:w], want[f][:w]
        inf = np.isinf(m)
        assert np.array_equal(np.isinf(g), inf) and np.all(g[inf] > 0), (what, f, g, m)
        assert np.all(np.abs(g[~inf].astype(np.float64) - m[~inf].astype(np.float64)) <= ulp32(m[~inf])), (what, f, g, m)
    c64 = res["centroid"]
    tol = 2.0 ** -23 * np.maximum(np.abs(c64), cfg["bw"])
    assert np.all(np.abs(stations["centroid_hz"][:w].astype(np.float64) - c64) <= tol), (what, stations["centroid_hz"][:w], c64)
    if chan is not None:
        chan = np.asarray(chan, dtype=np.float32)
        assert chan.shape == res["chan"].shape, what
        assert np.all(np.abs(chan.astype(np.float64) - res["chan"].astype(np.float64)) <= ulp32(res["chan"])), (what, "chan")


# ---- the fixed cases --------------------------------------------------------------------------------------------------------------------------

G64 = dict(rate=256000, n_bins=64, raster_hz=10000, bw=7000)                # D = 4000: fractional edges, C = 23
G256 = dict(rate=2400000, n_bins=256, raster_hz=100000, bw=100000)          # D = 9375: bw no multiple of D / 2, bands overlap by half, C = 21
G4096 = dict(rate=2400000, n_bins=4096, raster_hz=100000, bw=100000)        # C = 21, 342 bins a band
WIDE = dict(rate=2400000, n_bins=4096, raster_hz=2500, bw=1000)             # C = 959: up to four candidates a thread
T256 = dict(rate=1024000, n_bins=256, raster_hz=8000, bw=6000)              # D = 4000: a band is exactly the bins 2 c - 1 .. 2 c + 1, all weights 1; the
#                                                                             last candidate's band ends exactly at rate / 2 - D / 2; C = 127

# (name, configuration, n_blocks, n_streams, kind of input, exact ties expected)
CASES = [
    ("n64 b1 s1", config(**G64), 1, 1, "stations", False),
    ("n64 b3 s5 guard1 sep3", config(min_sep=3, dc_guard=1, **G64), 3, 5, "stations_dc", False),
    ("n256 b3 s5 guard3", config(dc_guard=3, **G256), 3, 5, "stations_dc", False),
    ("n256 b1 s1 guard0 dc", config(dc_guard=0, **G256), 1, 1, "stations_dc", False),
    ("n256 b1 s5 floor0", config(floor_permille=0, **G256), 1, 5, "stations", False),
    ("n256 b3 s1 floor1000", config(floor_permille=1000, threshold=0.5, **G256), 3, 1, "stations", False),
    ("n64 overflow", config(max_stations=2, **G64), 1, 5, "stations", False),
    ("n4096 b3 s5 guard3", config(dc_guard=3, max_stations=64, **G4096), 3, 5, "stations_dc", False),
    ("n4096 wide sep3", config(min_sep=3, max_stations=64, **WIDE), 1, 1, "stations", False),
    ("n4096 wide overflow b3", config(min_sep=1, max_stations=64, threshold=1.2, **WIDE), 3, 1, "stations", False),
    ("zeros", config(**G256), 3, 5, "zeros", False),
    ("sparse", config(max_stations=8, **T256), 1, 5, "sparse", False),
    ("plateau", config(**T256), 1, 1, "plateau", True),
    ("ties sep3 b3", config(min_sep=3, **T256), 3, 5, "ties", True),
    ("ties sep1 b1", config(min_sep=1, **T256), 1, 1, "ties", True),
]


def case_power(kind, cfg, n_blocks, n_streams, seed=1):
    """the input of a case, float32 [n_streams, n_blocks, n_bins], every stream with its own content; read-only"""
    N, R = cfg["n_bins"], cfg["rate"]
    pl = plan(cfg)
    C, cmax = pl["C"], pl["cmax"]
    out = np.zeros((n_streams, n_blocks, N), np.float32)
    k = np.arange(N)
    s = np.where(k < N // 2, k, k - N)
    f = s * (R / N)
    for st in range(n_streams):
        rng = np.random.default_rng(1000 * seed + 17 * st + N)
        if kind in ("stations", "stations_dc"):
            p = rng.uniform(0.5e-3, 1.5e-3, (n_blocks, N))
            n_st = min(C, 3 + (2 * st) % 5 + (4 if C > 100 else 0))
            cands = {0, C - 1} if st % 2 == 0 else set()
            cands |= set(int(x) for x in rng.choice(C, n_st, replace=False))
            for c in sorted(cands):
                amp = rng.uniform(0.02, 1.0)
                width = 0.5 * cfg["bw"] + 0.5 * R / N
                shape = np.exp(-0.5 * ((f - (c - cmax) * cfg["raster_hz"] - rng.uniform(-0.2, 0.2) * cfg["bw"]) / width) ** 2)
                p += amp * shape[None, :] * rng.uniform(0.8, 1.2, (n_blocks, 1))
            if kind == "stations_dc":
                p[:, np.abs(s) <= 2] += 5.0 * rng.uniform(0.8, 1.2)
            out[st] = p.astype(np.float32)
        elif kind == "zeros":
            pass
        elif kind == "sparse":                            # a few bins, the rest exactly zero: F = 0, snr = +inf
            for c in rng.choice(C, 3 + st, replace=False):
                out[st, :, (2 * (int(c) - cmax)) & (N - 1)] = np.float32(rng.uniform(0.1, 1.0))
        elif kind == "plateau":                           # T256: a floor of 2^-10, the bins of candidates 40 .. 47 at 1: equal Pc = 3 on all of them
            out[st] = np.float32(2.0 ** -10)
            lo, hi = 2 * (40 - cmax) - 1, 2 * (47 - cmax) + 1
            out[st, :, np.arange(lo, hi + 1) & (N - 1)] = 1.0
            out[st, :, (2 * (90 - cmax)) & (N - 1)] = 0.5
        elif kind == "ties":                              # T256: equal single-bin stations min_sep apart (the lower one stays) and min_sep + 1 apart (both stay,
            out[st] = np.float32(2.0 ** -10) * np.float32(1 + st)     # the lower one first), and one bin shared by two candidates (the lower one stays)
            ms = cfg["min_sep"]
            v = np.float32(0.25 * (1 + st))
            for c in (10, 10 + ms, 50, 50 + ms + 1):
                out[st, :, (2 * (c - cmax)) & (N - 1)] = v
            out[st, :, (2 * (100 - cmax) + 1) & (N - 1)] = np.float32(0.125)
            out[st, :, (2 * (0 - cmax)) & (N - 1)] = np.float32(3.0) * v       # candidates 0 and C - 1: the band's ends
            out[st, :, (2 * (C - 1 - cmax)) & (N - 1)] = np.float32(3.0) * v
        else:
            raise ValueError(kind)
    out.setflags(write=False)
    return out


# ---- the synthetic capture of the DC-spike and end-to-end tests -------------------------------------------------------------------------------

CAPTURE_RATE = 2400000
CAPTURE_CARRIERS = ((300000, 0.3), (-500000, 0.1), (900000, 0.03))       # (offset in Hz, amplitude of full scale)
CAPTURE_BLOCK_LEN, CAPTURE_BLOCKS = 16384, 2


def capture_bytes(n_bytes=CAPTURE_BLOCK_LEN * CAPTURE_BLOCKS, dc=0.05, noise=0.02, seed=5):
    """u8 IQ at 2.4 Msps: three FM carriers (a tone of 30 kHz deviation each), white noise and a DC offset, as a dongle delivers them"""
    n = np.arange(n_bytes // 2, dtype=np.float64)
    rng = np.random.default_rng(seed)
    z = np.full(n.size, dc * (1 + 0.5j), np.complex128)
    for q, (fc, amp) in enumerate(CAPTURE_CARRIERS):
        fm = 7000.0 + 3000.0 * q
        z += amp * np.exp(1j * (2 * np.pi * ((n * fc) % CAPTURE_RATE) / CAPTURE_RATE + (30000.0 / fm) * np.sin(2 * np.pi * fm * n / CAPTURE_RATE) + q))
    z += noise * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size)) / np.sqrt(2.0)
    out = np.empty(n_bytes, np.uint8)
    out[0::2] = np.clip(np.rint(z.real * 128.0 + 127.5), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(z.imag * 128.0 + 127.5), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def capture_config(n_bins=256, dc_guard=2):
    return config(CAPTURE_RATE, n_bins, 100000, 100000, dc_guard=dc_guard)
