"""Images and parameter sets that drive k_st_select (csrc/vo_shi_tomasi.hip) through every size class, chunk branch, conflict-list path and
limit instance ON PURPOSE.  tests/test_st_select_cases.py shows on the CPU that each case lands where it claims (on the oracle's response
map, with the brute-force model of tests/st_select_model.py); tests/test_gpu_st_select.py runs them on the GPU.  TEST INFRASTRUCTURE.

Sizes fixed on the CPU (valid candidates = 3 x 3 maxima above the quality threshold; uniform noise at block_size 3 has one per ~15 pixels):
    noise 600 x 440, seed 7      17 437 candidates   count classes up to 16 385; two chunks at min_distance 7 (3 044 corners from the first)
    noise 800 x 640, seed 11     34 134              three chunks at min_distance 12 and 20; first chunk fills 1 000 corners at 7
    blocks 500 x 400 (16 x 16)   44 665, 62 values   exact plateaus at block_size 31 (the fused NMS): rank 16 384 falls inside a run of equal values
    binary 160 x 120, seed 5      1 380              ties next to each other: pairs at distance 1 and sqrt 2, so 1.0 / 1.4 / 1.5 / 2.5 differ
    period-3 tile 600 x 448     264 180, 2 values    more raw candidates than the list holds: the one VO_E_CAPACITY exit
"""
import functools

import numpy as np

CHUNK = 16384


@functools.lru_cache(maxsize=None)
def image(kind, w, h, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        img = rng.integers(0, 256, (h, w))
    elif kind == "binary":                       # two grey levels: many equal responses next to each other
        img = rng.integers(0, 2, (h, w)) * 255
    elif kind == "blocks":                       # 16 x 16 blocks of two grey levels (tests/test_gpu_edges.py): exactly flat runs of the response
        img = np.kron(rng.integers(0, 2, (h // 16 + 1, w // 16 + 1)) * 200.0 + 20, np.ones((16, 16)))[:h, :w]
    elif kind == "flat":
        img = np.full((h, w), 128)
    elif kind == "tile3":                        # period 3 in x and y: a 3 x 3 box sum is the same at every interior pixel
        img = np.tile(rng.integers(0, 256, (3, 3)), (h // 3 + 1, w // 3 + 1))[:h, :w]
    elif kind == "frame":                        # an ordinary textured frame
        from vo_mi355x import synthetic as syn
        img = syn.make_sequence(1, w=w, h=h, seed=seed, margin=48)[0][0]
    else:
        raise ValueError(kind)
    img = np.ascontiguousarray(img, dtype=np.uint8)
    img.setflags(write=False)
    return img


NOISE_A = ("noise", 600, 440, 7)
NOISE_B = ("noise", 800, 640, 11)
PLATEAU = ("blocks", 500, 400, 1)
BINARY = ("binary", 160, 120, 5)
TILE = ("tile3", 600, 448, 3)


def case(name, img, md, maxc=0, q=1e-3, block=3, **land):
    """land: the landing condition(s) tests/test_st_select_cases.py asserts on the model:
       count = valid candidates; chunks = rank-ordered chunks the scan takes; later = a later chunk holds a candidate refused only by an earlier
       chunk's corner AND an accepted one; tie = the values at ranks 16383 / 16384 are equal (True) or differ (False); conf45 = candidates with
       exactly 4 and with more than 4 higher-ranked ones inside the radius; exact_kept = accepted pairs at exactly min_distance; corners = how
       many come out; sqrt2 / unit = candidate pairs at distance sqrt 2 / 1 exist; coarse = ceil(min_distance) cells would exceed 8192"""
    return dict(name=name, img=img, md=md, maxc=maxc, q=q, block=block, land=land)


# quality levels that leave exactly `count` valid candidates of NOISE_A (found by quality_for_count below; every target was reachable: the
# values at these ranks are distinct)
COUNT_QUALITY = {
    0: 1.0, 1: 0.9276076665075058, 2: 0.8536104527932733,
    1023: 0.48211718413360194, 1024: 0.48198503936320125, 1025: 0.4818906710377677,
    2048: 0.42449056389532647, 2049: 0.4243644240511489,
    4096: 0.3613244174129759, 4097: 0.3613126623149755,
    8192: 0.28661056124588025, 8193: 0.2866093966541279,
    16383: 0.15052809686783047, 16384: 0.15047694581445725, 16385: 0.15039284955221446,
}


def quality_for_count(resp, count):
    """-> a quality level q with exactly `count` candidates of resp above float32(float64(max) * q), or None where ties make it unreachable.
    The candidates above a threshold are the candidates of the unthresholded map whose value exceeds it (a pixel whose larger neighbour is
    zeroed is zeroed too), so the threshold is the value at rank `count`."""
    import st_select_model as m
    v, _ = m.candidates(resp, None, 1e-30)
    mx = np.float64(resp.max())
    if count == 0:
        return 1.0
    if count > len(v) or (count < len(v) and v[count] == v[count - 1]):
        return None
    lo = np.float64(v[count]) if count < len(v) else np.float64(v[-1]) * 0.5
    q = lo / mx
    for _ in range(8):                              # float32(mx * q) must land in [v[count], v[count - 1])
        t = np.float32(mx * q)
        if t < np.float32(lo):
            q = np.nextafter(q, np.inf)
        elif t >= v[count - 1]:
            q = np.nextafter(q, 0.0)
        else:
            return float(q)
    return None


COUNT_TARGETS = (0, 1, 2, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16383, 16384, 16385)


def count_cases():
    return [case("count%d-md%g" % (n, md), NOISE_A, md, 0, COUNT_QUALITY[n], count=n, **({"chunks": 2} if n > CHUNK and md >= 1 else {}))
            for n in COUNT_TARGETS for md in (7.0, 0.5)]


def chunk_cases():
    return [
        case("first-chunk-fills", NOISE_B, 7.0, 1000, chunks=1, over=CHUNK, corners=1000),
        case("two-chunks", NOISE_A, 7.0, 0, chunks=2, later=True, tie=False),
        case("three-chunks", NOISE_B, 12.0, 0, chunks=3, later=True, tie=False, over=2 * CHUNK),
        case("three-chunks-md20", NOISE_B, 20.0, 0, chunks=3, later=True, over=2 * CHUNK),
        case("plateau-first-fills", PLATEAU, 7.0, 300, 0.03, 31, chunks=1, over=CHUNK, tie=True, corners=300),
        case("plateau-three-chunks", PLATEAU, 7.0, 0, 0.03, 31, chunks=3, later=True, tie=True),
        case("plateau-two-chunks", PLATEAU, 3.0, 0, 0.03, 31, chunks=2, later=True, tie=True, corners=4096),
        case("no-rule-all", NOISE_B, 0.5, 0, chunks=1, over=CHUNK, corners=4096),
        case("no-rule-4096", NOISE_B, 0.0, 4096, chunks=1, over=CHUNK, corners=4096),
    ]


def conflict_cases():
    return [
        case("conflicts-4-and-more", NOISE_A, 7.0, 0, conf45=True),
        case("exact-distance-5", NOISE_A, 5.0, 0, exact_kept=True, conf45=True),
    ]


MD_VALUES = (0.0, 0.5, 0.999, 1.0, 1.4, 1.4142135, 1.5, 2.5, 6.5, 7.3, 7.5, 7.999)


def distance_cases():
    w, h = BINARY[1], BINARY[2]
    out = [case("md%g" % md, BINARY, md, 0, sqrt2=True, unit=True) for md in MD_VALUES]
    out += [case("md-above-side", BINARY, float(max(w, h) + 1), 0), case("md-above-diagonal", BINARY, float(np.hypot(w, h)) + 1.0, 0, corners=1),
            case("md1e6", BINARY, 1e6, 0, corners=1), case("md3e9", BINARY, 3e9, 0, corners=1), case("md-inf", BINARY, float("inf"), 0, corners=1)]
    for (w, h) in ((320, 240), (640, 480)):      # ceil(md) cells exceed the 8192 the kernel's grid holds: the cell is coarsened
        out += [case("md%g-%dx%d" % (md, w, h), ("binary", w, h, 6), md, 0, coarse=True, sqrt2=True, unit=True) for md in (1.0, 1.4, 2.5)]
    return out


def all_cases():
    return count_cases() + chunk_cases() + conflict_cases() + distance_cases()


# ---- the limited detection (vo_shi_tomasi_resident_limit) ----
LIMITS = (-3, 0, 1, 31, 32, 33, 100, 511, 512, 513, 2048)
LIMIT_MAX_CORNERS = (2048, 2049, 4096)          # the short-chunk instance (<= 2048), the large instance with a limit
LIMIT_SCENES = (                                  # name, image, block, quality, min_distance
    ("frame", ("frame", 320, 240, 4), 31, 0.03, 7.0),
    ("dense", ("noise", 320, 240, 9), 3, 1e-3, 1.0),            # > 4096 valid candidates, every one accepted
    ("plateau", ("blocks", 320, 240, 1), 31, 0.03, 3.0),
    ("dense-md20", ("noise", 320, 240, 9), 3, 1e-3, 20.0),      # few corners per short chunk: many passes
)


# ---- references, computed once per process and shared (the arrays are read-only) ----
_REF = {}


def reference(c):
    """-> (oracle corners cut at 4096, oracle response map, oracle candidate count, model Selection) of a case"""
    if c["name"] not in _REF:
        import st_select_model as m
        import vo_oracle as o
        img = image(*c["img"])
        ref, resp, rnc = o.good_features(img, None, maxCorners=c["maxc"], qualityLevel=c["q"], minDistance=c["md"], blockSize=c["block"], return_aux=True)
        sel = m.select(resp, None, c["maxc"], c["q"], c["md"])
        ref = ref[:m.OUT_CAP].copy()
        for a in (ref, resp, sel.corners):
            a.setflags(write=False)
        _REF[c["name"]] = (ref, resp, rnc, sel)
    return _REF[c["name"]]
