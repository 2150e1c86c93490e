"""TEST INFRASTRUCTURE: the lighting rotation of the relit chains (csrc/curved_light.inc, curved_relight_out_rows_kernel) restated in
float64 THROUGH ITS RECORDED ROUNDING POINTS, with a derived bound, for tests/test_relight_cpu.py and tests/test_gpu_relight.py.  Plain numpy.

    einsum('ab,nb->na', R, v) under fp16 autocast  =  half( fl32( fl32( h(R[a,0]) h(v[0]) + h(R[a,1]) h(v[1]) ) + h(R[a,2]) h(v[2]) ) )

h() rounds an fp32 value to half; the three products of half values are exact in fp32 (22 significant bits at most).

THE ERROR MODEL, u = 2^-24 (fp32), uh = 2^-11 (half), M_a = sum_b |h(R[a,b])| |h(v[b])|:
  inputs        h(R), h(v) are DETERMINED by the fp32 inputs: `rotate` applies them, they carry no error.  Against the UNROUNDED product R v
                (what a CPU run of the reference computes: its einsum stays fp32) they cost (2 uh + uh^2) sum_b |R[a,b]| |v[b]|: `unrounded_bound`.
  accumulation  two fp32 additions, each at most u times the magnitude of its result, itself at most M_a: 2 u M_a.
  output        one rounding to half of the fp32 sum y: uh |y| relative, and 2^-25 absolute for a result in half's subnormal range.
  together      |kernel - exact_a| <= 2 u M_a + uh (|exact_a| + 2 u M_a) + 2^-25                                              (`rotate`'s bound)

A DECIDED component is one whose exact value is further than 2 u M_a from every boundary between two adjacent half values: the fp32 sum then
rounds to the same half value as the exact one, and `value` is what the kernel holds, bit for bit.  An UNDECIDED component (about one in
2^13 / 2) may have been rounded to the neighbouring half value, `other`; a test holds such a row to either."""
import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11


def half(a):
    """fp32 values rounded to half, as float64."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def rodrigues(euler):
    """The float64 rotation matrix of a rotation vector, independently of the field's: I + sin(t) K + (1 - cos(t)) K^2."""
    v = np.asarray(euler, np.float64)
    t = np.linalg.norm(v)
    if t == 0:
        return np.eye(3)
    k = v / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def rotate(matrix32, v32):
    """matrix32 [3,3] fp32 (the values of the field's device buffer), v32 [N,3] fp32 -> dict: exact [N,3] (the float64 product of the half
    inputs), bound [N,3], value [N,3] (exact rounded to half: the kernel's vector where `decided`), other [N,3] (the neighbouring half value an
    undecided component may hold instead; = value where decided), decided [N,3] bool."""
    Rh, vh = half(np.asarray(matrix32, np.float32).reshape(3, 3)), half(v32)
    exact = vh @ Rh.T
    mag = np.abs(vh) @ np.abs(Rh).T
    acc = 2 * U * mag
    bound = acc + UH * (np.abs(exact) + acc) + 2.0 ** -25
    value = exact.astype(np.float16)
    lo, hi = (exact - acc).astype(np.float16), (exact + acc).astype(np.float16)
    decided = (lo == value) & (hi == value)
    other = np.where(lo != value, lo, hi).astype(np.float64)
    return dict(exact=exact, bound=bound, value=value.astype(np.float64), other=other, decided=decided)


def unrounded_bound(matrix, v):
    """|rotate(...)['exact'] - R v| for the UNROUNDED fp32 (or float64) operands: the two input roundings."""
    return (2 * UH + UH * UH) * (np.abs(np.asarray(v, np.float64)) @ np.abs(np.asarray(matrix, np.float64).reshape(3, 3)).T)


def variants(*rotated):
    """The vectors a kernel may hold for rows with undecided components: for each of the given rotate() results either `value` or `other` (all of a
    vector's undecided components together -- two in one vector is a 2^-24 event).  Yields tuples of [N,3] arrays, `value` everywhere first."""
    import itertools

    for pick in itertools.product((False, True), repeat=len(rotated)):
        yield tuple(r["other"] if p else r["value"] for r, p in zip(rotated, pick))
