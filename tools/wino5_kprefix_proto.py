"""Numpy (CPU, float64) statement of the forward 5x5 / stride-2 / pad-2 Winograd layer of csrc/winograd.hip with the zero blocks of the
transformed weights left out: four phase images X^(py,px)[r][q] = x[2r + py][2q + px] through F(4x4, 3x3), sub-kernels
g[u][v] = w[2u + py][2v + px] (zero beyond the 5 taps).  For py = 1 the third row of g is zero and the last row of G is [0 0 1], so
every plane (a, b) with a = 5 of U = G g G^T is zero for that phase; likewise px = 1 and b = 5: 23 of the 144 (phase, plane) blocks.

Layouts are the natural ones (plane 6 a + b; K = four phase blocks of C channels, phase 2 py + px).  The input transform leaves the 23
blocks of a tile row unwritten, the plane GEMMs step over them.  plan() restates wino_gemm_plan's partition (csrc/wino_gemm.hip): the
ranges are cut in the flat chunk list of the FULL K, exactly as when the zeros were multiplied, so every item is split where it was
and the float sums keep their bits; a workgroup multiplies the live chunks of its range only.
Run it to print the exactness of the form in float64 and the share of blocks kept."""
import numpy as np

BT = np.array([[1, 1.5, -2, -1.5, 1, 0], [0, -1, -2.5, -0.5, 1, 0], [0, 1, 0.5, -2.5, 1, 0], [0, -0.5, -1, 0.5, 1, 0], [0, 2, -1, -2, 1, 0],
               [0, 1, 1.5, -2, -1.5, 1]])
G = np.array([[1, 0, 0], [-1 / 3, -1 / 3, -1 / 3], [1 / 3, -1 / 3, 1 / 3], [1 / 15, 2 / 15, 4 / 15], [-16 / 15, 8 / 15, -4 / 15], [0, 0, 1]])
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -0.5, 0], [0, 1, 1, 4, 0.25, 0], [0, 1, -1, 8, -0.125, 1]])


def phase_mask(p):
    """bit 2 py + px is set where the weight block of phase (py, px) in plane p = 6 a + b is not zero (wino5_phase_mask)"""
    return (0x3 if p >= 30 else 0xF) & (0x5 if p % 6 == 5 else 0xF)


def live(p, ph):
    return bool((phase_mask(p) >> ph) & 1)


def pack(w):
    """w [Co, C, 5, 5] -> U [36][4 C][Co], every block computed (the dropped ones come out as zeros)"""
    Co, C = w.shape[:2]
    U = np.zeros((36, 4 * C, Co))
    for py in (0, 1):
        for px in (0, 1):
            g = np.zeros((Co, C, 3, 3))
            sub = w[:, :, py::2, px::2]
            g[:, :, :sub.shape[2], :sub.shape[3]] = sub
            u = np.einsum("au,ocuv,bv->abco", G, g, G)
            ph = 2 * py + px
            U[:, ph * C:(ph + 1) * C] = u.reshape(36, C, Co)
    return U


def input_transform(x):
    """x [H, W, C] -> V [th * tw][36][4 C]; what the kernel does not store stays NaN"""
    H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    th, tw = -(-Ho // 4), -(-Wo // 4)
    V = np.full((th * tw, 36, 4 * C), np.nan)
    for py in (0, 1):
        for px in (0, 1):
            X = np.zeros((4 * th + 2, 4 * tw + 2, C))          # phase image with its pad-1 border
            ph = x[py::2, px::2]
            X[1:1 + ph.shape[0], 1:1 + ph.shape[1]] = ph
            for ty in range(th):
                for tx in range(tw):
                    d = X[4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6]
                    v = np.einsum("ar,rsc,bs->abc", BT, d, BT)
                    for a in range(6):
                        for b in range(6):
                            if (a < 5 or py == 0) and (b < 5 or px == 0):      # the kernel's store predicate
                                V[ty * tw + tx, 6 * a + b, (2 * py + px) * C:(2 * py + px + 1) * C] = v[a, b]
    return V, (th, tw, Ho, Wo)


def conv_wino5(x, w):
    """-> y [Ho, Wo, Co]: input transform, per-plane contraction over the live phase blocks only, output transform"""
    C, Co = x.shape[2], w.shape[0]
    U = pack(w)
    V, (th, tw, Ho, Wo) = input_transform(x)
    M = np.zeros((th * tw, 36, Co))
    for p in range(36):
        for ph in range(4):
            if live(p, ph):
                M[:, p] += V[:, p, ph * C:(ph + 1) * C] @ U[p, ph * C:(ph + 1) * C]
    y = np.zeros((4 * th, 4 * tw, Co))
    for ty in range(th):
        for tx in range(tw):
            m = M[ty * tw + tx].reshape(6, 6, Co)
            y[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = np.einsum("ka,abo,lb->klo", AT, m, AT)
    return y[:Ho, :Wo]


def conv_direct(x, w):
    """x [H, W, C], w [Co, C, 5, 5], stride 2 pad 2 -> [Ho, Wo, Co]"""
    H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((2 * Ho + 4, 2 * Wo + 4, C))
    xp[2:2 + H, 2:2 + W] = x
    y = np.zeros((Ho, Wo, w.shape[0]))
    for i in range(5):
        for j in range(5):
            y += xp[i:i + 2 * Ho:2, j:j + 2 * Wo:2] @ w[:, :, i, j].T
    return y


TILES = {3: (64, 64), 4: (128, 128), 5: (128, 256), 6: (160, 128), 7: (96, 128)}


def plan(T, C, Cout, tile, slots, cus=256):
    """wino_gemm_plan for a forward 5x5 / stride-2 layer -> (ranges, items, live): the flat chunk range [begin, end) of every workgroup and
    of every item in the kernel's plane-major order -- both exactly those of the full K -- and per flat chunk whether it is multiplied"""
    if tile == 5 and Cout % 256:
        tile = 4
    if tile not in TILES or Cout % 128:
        tile = 3
    BM, BN = TILES[tile]
    MT, NTN = -(-T // BM), Cout // BN
    nch, q = 4 * C // 32, C // 32
    n_items = MT * NTN * 36
    total = n_items * nch
    Gw = min(n_items, slots)
    if cus < Gw < slots:
        Gw = Gw // cus * cus
    per, rem = divmod(total, Gw)
    first = lambda w: w * per + min(w, rem)
    ranges = [(first(w), first(w + 1)) for w in range(Gw)]
    items = [(i * nch, (i + 1) * nch) for i in range(n_items)]
    alive = np.concatenate([np.repeat([live(i // (MT * NTN), ph) for ph in range(4)], q) for i in range(n_items)])
    return ranges, items, alive


def workgroups_per_item(ranges, items, alive):
    """for every item, the number of workgroups that multiply at least one of its chunks"""
    csum = np.concatenate([[0], np.cumsum(alive)])
    starts = np.array([r[0] for r in ranges])
    out = []
    for b, e in items:
        lo = np.searchsorted(starts, b, side="right") - 1       # the range that holds flat chunk b
        hi = np.searchsorted(starts, e - 1, side="right") - 1
        out.append(sum(1 for w in range(lo, hi + 1) if csum[min(ranges[w][1], e)] - csum[max(ranges[w][0], b)] > 0))
    return np.array(out)


def main():
    rng = np.random.RandomState(0)
    for H, W, C, Co in ((9, 11, 3, 2), (16, 24, 4, 3)):
        x, w = rng.randn(H, W, C), rng.randn(Co, C, 5, 5)
        ref = conv_direct(x, w)
        print("H %d W %d: max |wino - direct| = %.1e of %.2f" % (H, W, np.abs(conv_wino5(x, w) - ref).max(), np.abs(ref).max()))
    kept = sum(bin(phase_mask(p)).count("1") for p in range(36))
    print("blocks multiplied: %d of 144 (%.1f %% less)" % (kept, 100 - 100.0 * kept / 144))


if __name__ == "__main__":
    main()
