"""The grid of the kernel-edge tests of csrc/vq.hip, shared by tests/test_vq_edges_gpu.py (which runs it on the device) and
tests/test_vq_ref_cpu.py (which checks its preconditions on the host).  Every case is generated from its name's seed.

Search cases are named after the kernel instantiation they are there for; search_kernel() restates the dispatch rule of
alvq_vq_argmin_f32 so that the table can be checked against it.  The labels of the gather / backward cases are drawn, never
computed, so that K can be large without a K-wide float64 distance matrix."""
import itertools

import numpy as np

import vq_ref as R

F32 = np.float32
TWO_FRAG_N = 128 * 512 + 65


# ------------------------------------------------------------------------------------------------------ dispatch, restated
def search_kernel(n, k, d, vq_reg=1):
    """The kernel alvq_vq_argmin_f32 launches: x rows in registers for D <= 256 (option vq_reg), in 32-dim chunks nd = 2, 4
    or 8, two 16-row fragments a wave where nd < 8 and N >= 128 * 512; otherwise x stationary in LDS, 8 waves from D = 128
    up where 128 rows fit 160 KiB beside the codebook tile, else 4."""
    if d <= 256 and vq_reg:
        nd = 2 if d <= 64 else (4 if d <= 128 else 8)
        return "reg<%d,%d>" % (nd, 2 if nd != 8 and n >= 128 * 512 else 1)
    dp = (d + 31) // 32 * 32
    xstr = dp + ((2 - dp % 32) + 32) % 32
    wide = d >= 128 and (128 * xstr + 128 * 34) * 4 <= 160 * 1024
    return "lds<8>" if wide else "lds<4>"


# (kernel the case is there for, the vq_reg that reaches it, N, K, D)
def _grid(kernel, reg, ns, ks, ds):
    return [(kernel, reg, n, k, d) for n, k, d in itertools.product(ns, ks, ds)]


SEARCH = (
    _grid("reg<2,1>", 1, (1, 63, 65, 777), (1, 16, 130), (1, 3, 33, 64))
    + _grid("reg<2,2>", 1, (TWO_FRAG_N,), (130,), (8, 33))          # 33: the codebook tile through scalar loads
    + _grid("reg<4,1>", 1, (777,), (513,), (65, 100, 128))
    + _grid("reg<4,2>", 1, (TWO_FRAG_N,), (130,), (68, 128))
    + _grid("reg<8,1>", 1, (129,), (1000,), (129, 200, 255, 256))
    + _grid("lds<4>", 0, (65,), (130,), (4, 100))
    + _grid("lds<4>", 1, (65,), (130,), (257, 300, 512))             # D > 256: LDS whatever the option
    + _grid("lds<8>", 0, (129, 300), (513,), (128, 200, 256))
    + [("reg<2,1>", 1, 300, 4096, 32)]                               # the default codebook size
)
FAMILIES = ("lattice", "gauss", "init")
SEPARATED_MIN_D = 8        # the planted ("separated") family is run where D >= 8: see search_case


def search_id(c):
    return "%s_n%d_k%d_d%d" % (c[0].replace("<", "").replace(">", "").replace(",", "x"), c[2], c[3], c[4])


def regs_of(case):
    """The vq_reg values a case is run with: both where D <= 256."""
    return (1, 0) if case[4] <= 256 else (1,)


def case_seed(name):
    return 2000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100000


# the bitwise-equal code rows, in sets without a common code (a code in two pairs would make a triple of the two):
#   15|16 two lanes of one accumulator group's neighbours     16|32 one lane, two accumulator groups (ni)
#   127|128 two 128-code tiles                                0|K-1 first and last code
#   two codes of the ragged last tile
def tie_variants(k):
    out = []
    for pairs in ([(15, 16), (127, 128)], [(16, 32), (0, k - 1)]):
        pairs = [(a, b) for a, b in pairs if a < b < k]
        if pairs:
            out.append(pairs)
    k0 = (k - 1) // 128 * 128
    if k % 128 and k - k0 >= 2:
        out.append([(k0, k0 + 1)])
    return out or [[]]


def lattice_case(case, variant):
    """-> (x, e, planted): integers in [-16, 16]; planted = [(row, lo, hi, kind)], kind "tie" (e[hi] is e[lo] bit for bit and
    the row equals both: distance 0) or "equidistant" (two unequal codes at distance 1 from the row)."""
    _, _, n, k, d = case
    rs = np.random.RandomState(case_seed(search_id(case)) + variant)
    x = rs.randint(-16, 17, (n, d)).astype(F32)
    e = rs.randint(-16, 17, (k, d)).astype(F32)
    pairs = tie_variants(k)[variant]
    planted = []
    rows = [r for r in dict.fromkeys([(37 * j + 5) % n for j in range(8)] + [n - 1, 0])]
    for lo, hi in pairs:
        e[hi] = e[lo]
    taken = {c for p in pairs for c in p}
    free = [c for c in range(k) if c not in taken][:2]
    for lo, hi in pairs:
        for _ in range(2):
            if rows:
                r = rows.pop(0)
                x[r] = e[lo]
                planted.append((r, lo, hi, "tie"))
    if len(free) == 2 and rows:
        a, b = free
        r = rows.pop(0)
        e[b] = e[a]
        e[a, 0], e[b, 0] = 0.0, 2.0
        x[r] = e[a]
        x[r, 0] = 1.0
        planted.append((r, a, b, "equidistant"))
    return x, e, planted


def search_case(case, family):
    """gauss: x ~ N(0, 1), codebook N(0, 0.8);  init: codebook U(+-1/K), the rounding-dominated regime;  separated: gauss with
    every row 0.01 N(0, 1) away from a drawn code, so that the float64 margin decides every index (checked on the host)."""
    _, _, n, k, d = case
    rs = np.random.RandomState(case_seed(search_id(case) + family))
    x = rs.randn(n, d).astype(F32)
    if family == "init":
        e = ((rs.rand(k, d) * 2.0 - 1.0) / k).astype(F32)
    else:
        e = (rs.randn(k, d) * 0.8).astype(F32)
    if family == "separated":
        x = (e[rs.randint(0, k, n)] + 0.01 * x).astype(F32)
    return x, e


def separated_cases():
    return [c for c in SEARCH if c[4] >= SEPARATED_MIN_D and c[3] >= 2]


# the non-finite rows: (case, x row with a NaN, x row with +inf, code row with +inf); the rows sit inside a 16-row fragment,
# for the two-fragment kernel in fragment 1 of a wave (rows 16 .. 31 of its 32)
NONFINITE = [
    (("reg<2,1>", 1, 777, 130, 33), 16 * 3 + 7, 16 * 3 + 9, 77),
    (("reg<4,2>", 1, TWO_FRAG_N, 130, 68), 128 * 3 + 32 + 16 + 7, 128 * 3 + 32 + 16 + 9, 129),
    (("reg<8,1>", 1, 129, 1000, 200), 16 * 5 + 7, 16 * 5 + 9, 999),
    (("lds<4>", 1, 65, 130, 300), 16 + 7, 16 + 9, 15),
]


# ------------------------------------------------------------------------------- gather, loss, backward: drawn labels
# (name, N, K, D, draw, argument)
#   uniform            drawn labels (codes that get no row stay without one)
#   hot                code min(3, K - 1) owns the first 7/8 of the rows: several flushes of the gather list
#   seg                code 1 owns exactly arg[0] consecutive rows from row arg[1] on and no other; the rest uniform over the
#                      other codes.  1024 rows fill one chunk (no flush), 1025 flush after the second, 2048 fill the list
#                      to its last slot, 2049 go one past it
GATHER = [
    ("n1", 1, 1, 1, "uniform", None),
    ("n3_k7_d6", 3, 7, 6, "uniform", None),                       # fewer rows than loss workgroups; codes without a row
    ("n1023_d86_hot", 1023, 7, 86, "hot", None),
    ("n1025_d128", 1025, 7, 128, "uniform", None),                # one and two rows a workgroup
    ("n4097_d260_hot", 4097, 7, 260, "hot", None),                # 65 lanes, three groups, 61 idle threads; P = 1
    ("n8193_d512_hot", 8193, 7, 512, "hot", None),                # P = 2: segments of 5120 and 3073 rows
    ("n8193_k1_d129", 8193, 1, 129, "uniform", None),             # one code owns everything
    ("n65537_d255", 65537, 7, 255, "uniform", None),              # P = 16, rows_per_part 5120: segments 13 .. 15 empty
    ("n65537_d4_hot", 65537, 7, 4, "hot", None),
    ("n70001_k8192_d4_hot", 70001, 8192, 4, "hot", None),         # the last K with the histogram in LDS
    ("n70001_k8193_d6", 70001, 8193, 6, "uniform", None),         # the first K with global atomics
    ("n65537_k16384_d1", 65537, 16384, 1, "uniform", None),       # about 300 codes without a row
    ("n70001_k16384_d4_hot", 70001, 16384, 4, "hot", None),
    ("seg1024_d4", 8193, 7, 4, "seg", (1024, 0)),
    ("seg1025_d6", 8193, 7, 6, "seg", (1025, 5120)),              # 5120: the first row of segment 1
    ("seg2048_d128", 8193, 7, 128, "seg", (2048, 5120)),
    ("seg2049_d86", 8193, 7, 86, "seg", (2049, 0)),
]
ONEHOT = [(1, 1), (1, 7), (777, 1), (1025, 130), (4097, 1100)]   # the last: N K > 2048 * 256 * 8, the grid-stride loop wraps
BETA = 0.25


def hot_code(k):
    return min(3, k - 1)


def make_idx(seed, n, k, draw, arg):
    rs = np.random.RandomState(seed)
    if draw == "seg":
        count, start = arg
        others = np.array([c for c in range(k) if c != 1])
        idx = others[rs.randint(0, k - 1, n)]
        idx[start:start + count] = 1
        return idx.astype(np.int64)
    idx = rs.randint(0, k, n).astype(np.int64)
    if draw == "hot":
        idx[:n - n // 8] = hot_code(k)
    return idx


def gather_case(case, family):
    """-> (x, e, idx): lattice (integers in [-16, 16]) or gauss (x ~ N(0, 1), codebook N(0, 0.8))."""
    name, n, k, d, draw, arg = case
    seed = case_seed(name + family)
    rs = np.random.RandomState(seed)
    if family == "lattice":
        x = rs.randint(-16, 17, (n, d)).astype(F32)
        e = rs.randint(-16, 17, (k, d)).astype(F32)
    else:
        x = rs.randn(n, d).astype(F32)
        e = (rs.randn(k, d) * 0.8).astype(F32)
    return x, e, make_idx(seed + 1, n, k, draw, arg)


def exact_grad_loss(n, d):
    """-> (grad_loss, se): a float32 grad_loss whose float32 product with float32(2 / (N D)) is a power of two, se.  On the
    lattice every term se (e - x) of the codebook gradient and every sum of them is then exact in float32, in any order, as
    long as rows_of_a_code * 32 < 2^24; with beta = 0.25, sx = se / 4 as well."""
    ce = F32(2.0 / (float(n) * float(d)))
    p0 = int(np.floor(np.log2(float(ce))))
    for p in (p0, p0 + 1, p0 - 1):
        target = F32(2.0 ** p)
        gl = F32(float(target) / float(ce))
        lo = gl
        for _ in range(8):
            lo = np.nextafter(lo, F32(0.0))
        c = lo
        for _ in range(17):
            if F32(c * ce) == target:
                return c, target
            c = np.nextafter(c, F32(np.inf))
    raise AssertionError("no grad_loss makes se a power of two for N=%d D=%d" % (n, d))


def lattice_base(seed, k, d, se):
    """The accumulate form's base: integers in [-16, 16] times se."""
    return (np.random.RandomState(seed).randint(-16, 17, (k, d)) * float(se)).astype(F32)
