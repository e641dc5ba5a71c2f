"""Live work per stream-K range of a 5x5 / stride-2 layer's plane GEMMs, before and after the item map (csrc/wino_balance.hip).

    python tools/wino_balance.py                      # conv2 and conv3 at 16 pairs
    python tools/wino_balance.py T K Cout tile [G]    # one GEMM shape (K = 4 Cin)

G: the workgroups of the launch.  Given, nothing but host arithmetic runs (no GPU needed); left out, the library asks the device for
the G a launch would take.  The figures are recomputed here from the table, not read from its header."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mx-deepim_amd"))

FLAGSHIP = {"conv2": (19200, 256, 128, 4), "conv3": (4800, 512, 256, 5)}   # 16 pairs: T = 16 * 30 * 40, 16 * 15 * 20


def phase_mask(p):
    return (0x3 if p >= 30 else 0xF) & (0x5 if p % 6 == 5 else 0xF)


def live_per_range(table, hdr):
    nch, G, per, rem = hdr["nch"], hdr["G"], hdr["per"], hdr["rem"]
    q, per_plane = nch // 4, hdr["items"] // 36
    chunk_live = np.array([[(phase_mask(p) >> (ch // q)) & 1 for ch in range(nch)] for p in range(36)])
    flat = chunk_live[np.asarray(table) // per_plane].reshape(-1)
    first = [w * per + min(w, rem) for w in range(G + 1)]
    return np.array([flat[first[w]:first[w + 1]].sum() for w in range(G)])


def report(name, T, K, Cout, tile, G=0):
    from lib.hip import ops

    hdr, table = ops.wino_item_map_plan(T, K, Cout, tile, G)
    before, after = live_per_range(np.arange(hdr["items"]), hdr), live_per_range(table, hdr)
    planes = [len(set((table[s] // (hdr["items"] // 36)) for s in range(f // hdr["nch"], -(-l // hdr["nch"]))))
              for f, l in ((w * hdr["per"] + min(w, hdr["rem"]), (w + 1) * hdr["per"] + min(w + 1, hdr["rem"])) for w in range(hdr["G"]))]
    print("{}: T {} K {} Cout {} tile {}  G {}  flat/range {}{}  items {} of {} chunks".format(
        name, T, K, Cout, hdr["tile"], hdr["G"], hdr["per"], "+1" if hdr["rem"] else "", hdr["items"], hdr["nch"]))
    for tag, v in (("before", before), ("after", after)):
        print("  live/range {:6s} min {:4d}  mean {:6.1f}  max {:4d}".format(tag, int(v.min()), v.mean(), int(v.max())))
    print("  slots moved {}  planes per range max {} mean {:.2f}  (header: live max {} -> {})".format(
        hdr["moved"], max(planes), float(np.mean(planes)), hdr["live_max_before"], hdr["live_max_after"]))


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    if args:
        report("gemm", *args)
    else:
        for name, shape in FLAGSHIP.items():
            report(name, *shape)
