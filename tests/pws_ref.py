"""Reference of the phase-weighted stack ("Phase-weighted stack"; csrc/pws.h, csrc/dvh_pws.hip), its two
bounds with their derivations, and the cases the host and GPU tests share.

hilbert_imag is the closed-form circular convolution in np.longdouble, written from the transform's definition and not
from pws.h's half-angle forms; tests/test_pws_host.py holds it to scipy.signal.hilbert.  pws is the definition in
float64 from it:

    a_j = g_j + i h_j,  p_j = a_j / |a_j| (0 where a_j = 0),  lin = sum_j g_j / m,  c = |sum_j p_j| / m,
    out = lin * c**power
"""
import numpy as np

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))
WS = [1, 2, 3, 7, 8, 64, 65, 499, 500, 1023, 1024]  # the passes' lag counts (one case each)
N_PASS, R = 11, 3
MS = [1, 2, 7, 8, 9, 17, 31]  # both sides of the kernel's 4-load group, several groups plus every tail length
POWERS = [0.0, 1.0, 2.0, 3.5]
DEAD = (3, 1)  # (pass, row) that is all zero
NEG = (7, 2)  # pass 7 is the exact negation of pass 2


def taps(n):
    """k[0..n): imag(hilbert(x))[t] = sum_s k[(t - s) mod n] x[s], in longdouble."""
    k = np.zeros(n, dtype=LD)
    if n == 1:
        return k
    i = np.arange(1, n)
    th = PI * i.astype(LD) / LD(n)
    if n % 2 == 0:
        k[1:] = np.where(i % 2 == 1, LD(2) / LD(n) * np.cos(th) / np.sin(th), LD(0))
        k[n // 2] = 0  # cot(pi / 2), which the rounded pi / 2 misses by 1e-20: at n = 2 it is the only tap

    else:
        sign = np.where(i % 2 == 0, LD(1), LD(-1))  # cos(pi i)
        k[1:] = (np.cos(th) / np.sin(th) - sign / np.sin(th)) / LD(n)
    return k


_CIRC = {}


def _circulant(n):
    if n not in _CIRC:
        t = np.arange(n)
        _CIRC[n] = taps(n)[(t[:, None] - t[None, :]) % n]
    return _CIRC[n]


def hilbert_imag(x, n):
    """imag(scipy.signal.hilbert(x[..., :n])) over the last axis as longdouble [..., n]."""
    x = np.asarray(x)[..., :n].astype(LD)
    return x @ _circulant(n).T


def tap_l1(n):
    return float(np.abs(taps(n)).sum())


def hilbert_bound(ref, n, x_inf):
    """|H - ref| <= 2^-24 |ref| + (n + 2) 2^-52 ||k||_1 ||x||_inf per element: the one rounding of the float64 sum to
    float32 (half an ulp, relative 2^-24), and the float64 sum itself -- n products added in sequence carry at most
    n rounding errors of 2^-53 relative to the sum of magnitudes, which ||k||_1 ||x||_inf bounds; a tap within 2 ulp of
    its value (one quotient and one tangent of an argument that is itself a rounded product) adds 2 * 2^-52 of it.
    (n + 2) 2^-52 covers both with a factor 2 to spare."""
    return 2.0 ** -24 * np.abs(np.asarray(ref, dtype=np.float64)) + (n + 2) * 2.0 ** -52 * tap_l1(n) * float(x_inf)


def analytic(G, w_of=None):
    """H [n, R, W] float64 of passes G [n, R, W] (float32): pass j transformed over its own w_of[j] lags (default: all
    W), 0 beyond."""
    G = np.asarray(G, dtype=np.float32)
    n, W = G.shape[0], G.shape[-1]
    w_of = np.full(n, W) if w_of is None else np.asarray(w_of)
    H = np.zeros(G.shape, np.float64)
    for j in range(n):
        H[j, ..., :w_of[j]] = hilbert_imag(G[j], int(w_of[j])).astype(np.float64)
    return H


def parts(G, H, sel):
    """(lin, c, mean_j |g_j|) in float64 of one draw ``sel`` of passes G [n, R, W] (float32) with H = analytic(G)."""
    acc_g = np.zeros(G.shape[1:], np.float64)
    acc_p = np.zeros(G.shape[1:], np.complex128)
    acc_abs = np.zeros(G.shape[1:], np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in sel:
            j = int(j)
            g = G[j].astype(np.float64)
            a = g + 1j * H[j]
            mag = np.abs(a)
            acc_p += np.where(mag > 0, a / np.where(mag > 0, mag, 1.0), np.where(np.isnan(mag), np.nan, 0.0))
            acc_g += g
            acc_abs += np.abs(g)
    m = len(sel)
    return acc_g / m, np.abs(acc_p) / m, acc_abs / m


def weighted(lin, c, power):
    return lin * c ** power if power != 0 else lin


def pws(G, sel, power, w_of=None):
    """The phase-weighted stack of one draw, float64 [R, W]."""
    lin, c, _ = parts(G, analytic(G, w_of), sel)
    return weighted(lin, c, power)


def pws_bound(m, power, mean_abs_g):
    """|out - ref| <= 2^-23 ((m + 2)(1 + power) + 6) mean_j |g_j| per element.  With e = 2^-23 (one float32 ulp of 1,
    twice the unit roundoff, which leaves room for the second-order terms) and M = mean_j |g_j| >= |lin|:

      lin   m - 1 adds of a sum whose partial sums stay below m M, and one division: |d lin| <= m (e / 2) M, counted
            as (m + 2) e M;
      c     each phasor carries three roundings (the norm, its reciprocal root, the product) on a value of at most 1,
            and h's own rounding turns the phase by at most 2^-25; each of the two phasor sums adds m - 1 roundings
            on partial sums of at most m; after the division by m, |d c| <= (m + 2) e, and the magnitude, its square
            root and the division add 3 e on c <= 1;
      out   c**power has slope at most power on [0, 1] (power >= 1), so |lin| |d c**power| <= power (m + 2) e M + 3 e M;
            |d lin| c**power <= (m + 2) e M; the weight's product and powf add at most 3 e M.

    Sum: ((m + 2)(1 + power) + 6) e M.  power = 0 is exact (the linear stack bit for bit) and inside the bound."""
    return 2.0 ** -23 * ((m + 2) * (1.0 + power) + 6.0) * np.asarray(mean_abs_g, dtype=np.float64)


def passes(W, seed=0):
    """11 passes of 3 rows of W lags: one dead row, one pass the exact negation of another."""
    G = np.random.default_rng(4000 + W + seed).standard_normal((N_PASS, R, W)).astype(np.float32)
    G[DEAD[0], DEAD[1]] = 0.0
    G[NEG[0]] = -G[NEG[1]]
    return G


def selection(rng, B, m):
    sel = rng.integers(0, N_PASS, size=(B, m)).astype(np.int32)
    if m >= 2:
        sel[0, 1] = sel[0, 0]  # a repeated pass in every size that has room for one
    return sel


def draws(W):
    """{(m, B): sel [B, m]} for m in MS, B in (1, 6), as one flat table with offsets that are neither monotone nor
    disjoint: (flat, {(m, B): (off [B], cnt [B])}, {(m, B): sel})."""
    rng = np.random.default_rng(W)
    sels = {(m, B): selection(rng, B, m) for m in MS for B in (1, 6)}
    flat, tables = [], {}
    for key in sorted(sels, key=lambda k: (-k[0], k[1])):  # large draws first: later offsets are not ascending in m
        m, B = key
        base = sum(len(x) for x in flat)
        flat.append(sels[key].reshape(-1))
        off = base + np.arange(B, dtype=np.int32) * m
        tables[key] = (off[::-1].copy(), np.full(B, m, np.int32))  # rows stored back to front: off descends
        sels[key] = sels[key][::-1].copy()
    flat = np.concatenate(flat).astype(np.int32)
    # a draw that overlaps two others: it starts 5 entries into one stored row and runs 5 entries into the next
    m, B = 7, 6
    off, cnt = tables[(m, B)]
    off = off.copy()
    off[2] = off[3] + 5
    tables[(m, B)] = (off, cnt)
    sels[(m, B)] = np.stack([flat[o:o + c] for o, c in zip(off, cnt)])
    return flat, tables, sels


_CASES = {}


def case(W):
    """(G, analytic(G), flat, tables, sels, {(m, B): [parts of every row]}) of one lag count, computed once and shared
    by the host and GPU tests (read-only)."""
    if W not in _CASES:
        G = passes(W)
        H = analytic(G)
        flat, tables, sels = draws(W)
        stats = {key: [parts(G, H, row) for row in sel] for key, sel in sels.items()}
        for a in (G, H, flat):
            a.setflags(write=False)
        _CASES[W] = (G, H, flat, tables, sels, stats)
    return _CASES[W]
