"""Prices, on the CPU, what the SOURCE-HIT classification of the edge ring kernel saves (round 11; the numbers quoted in
profiles/r11_edge/README.md; built on tools/edge_ring_sim.py, the same two-ring model with entries in (j, k, scene, i) order).

Sample 0 of a neighbour edge k -> i is the source node, so "obstacle m is a hard hit at sample 0" (d2[0] <= 16) depends on
(scene, column, m, k) only and the pair contributes exactly w_coll.  Table 1: how many (edge, obstacle) scans and ring entries
that resolves.  Table 2: wave-level scans (a round of the one-obstacle ring is one scan, a round of the several-obstacle ring as
many as its longest entry) for three classifications:

  today   every obstacle in reach is scanned;
  ideal   entries classified by the scans still needed, hits dropped from every entry (needs the hits' places in the sum beside
          every entry: more than a ring entry holds);
  built   no scan left: stored from the dense pass; one scan and at most one hit on either side of it: the one-obstacle ring (two
          flag bits); everything else: the several-obstacle ring with its whole mask, hits scanned like the rest.

(tools/edge_ring_sim.py is a script that prices its one configuration while it is imported, so its model is restated here, in
the same terms, as a function that is called once per configuration.)

Usage: python tools/edge_source_hit_sim.py                                  every combination the README quotes
       python tools/edge_source_hit_sim.py cfg2|cfg5 [scenes] [waves_per_tile] [corridor|survey|worst]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emplanner_carla_amd import scenes as S

def rounds(*rings):
    """wave-level scans of rings given as arrays of scans per entry (entries popped 64 at a time, in order)"""
    tot = 0
    for q in rings:
        if len(q):
            tot += int(np.concatenate([q, np.zeros((-len(q)) % 64, int)]).reshape(-1, 64).max(1).sum())
    return tot



def price(name, B, WPT, dist):
    """one configuration, batch size, wavefronts a tile (block size: they share a tile's columns) and obstacle layout"""
    cfg = {"cfg2": S.CFG2, "cfg5": S.CFG5}[name]
    b = S.make_batch(range(B), cfg, start_ahead=S.BENCH_START_AHEAD, dist=dist)
    row, col, ss, sl = cfg.row, cfg.col, cfg.sample_s, cfg.sample_l
    Sx = 64 // row
    tiles = B // Sx
    lat = ((row + 1) / 2 - 1 - np.arange(row)) * sl
    llo, lhi = np.minimum.outer(lat, lat), np.maximum.outer(lat, lat)          # [k][i]
    ps = b.sl_start[:, 0]
    s0 = ps[:, None] + np.arange(1, col)[None, :] * ss                          # B, col-1
    s9 = s0 + 9 * ss / 10
    os_, ol_ = b.sl_obs_s, b.sl_obs_l                                           # B, m
    valid = np.arange(os_.shape[1])[None, :] < b.n_obs[:, None]
    dx = np.maximum(np.maximum(s0[:, :, None] - os_[:, None, :], os_[:, None, :] - s9[:, :, None]), 0)    # B, col-1, m
    scans = hits = entries = ent_none = ent_one = ent_one_built = 0
    wave = {"today": 0, "ideal": 0, "built": 0}
    lane = {"today": 0, "ideal": 0, "built": 0}
    for tl in range(tiles):
        s_ = slice(tl * Sx, (tl + 1) * Sx)
        dy = np.maximum(np.maximum(llo[None, None] - ol_[s_, :, None, None], ol_[s_, :, None, None] - lhi[None, None]), 0)     # S, m, k, i
        box = (dx[s_][:, :, :, None, None] ** 2 + dy[:, None] ** 2 < 36.5) & valid[s_][:, None, :, None, None]         # S, col-1, m, k, i
        d_lon, d_lat = os_[s_][:, None, :, None] - s0[s_][:, :, None, None], ol_[s_][:, None, :, None] - lat[None, None, None, :]
        H = (d_lon * d_lon + d_lat * d_lat <= 16.0)[..., None] & box                                                   # S, col-1, m, k, (i)
        left = box & ~H
        c_pass, c_scan = box.sum(2), left.sum(2)                                                                       # S, col-1, k, i
        # the built form: one scan left, at most one hit below and one above it in slot order
        first = np.where(left.any(2), left.argmax(2), 0)                                                               # S, col-1, k, i
        m_idx = np.arange(box.shape[2])[None, None, :, None, None]
        below, above = (H & (m_idx < first[:, :, None])).sum(2), (H & (m_idx > first[:, :, None])).sum(2)
        ring0 = (c_scan == 1) & (below <= 1) & (above <= 1)
        scans += int(c_pass.sum()); hits += int(H.sum())
        entries += int((c_pass > 0).sum()); ent_none += int(((c_pass > 0) & (c_scan == 0)).sum())
        ent_one += int((c_scan == 1).sum()); ent_one_built += int(ring0.sum())
        for w in range(WPT):
            o = lambda x: np.transpose(x[:, w::WPT], (1, 2, 0, 3)).reshape(-1)                                         # (j, k, scene, i)
            p, c, r0 = o(c_pass), o(c_scan), o(ring0)
            wave["today"] += rounds(p[p == 1], p[p > 1]); lane["today"] += int(p.sum())
            wave["ideal"] += rounds(c[c == 1], c[c > 1]); lane["ideal"] += int(c.sum())
            wave["built"] += rounds(c[r0], p[(c > 0) & ~r0]); lane["built"] += int(c[r0].sum() + p[(c > 0) & ~r0].sum())

    n = tiles * Sx
    print(f"{cfg.name} {dist}: {n} scenes, S = {Sx}, {WPT} wavefronts a tile")
    print(f"  scans a scene {scans / n:.0f}; hard at sample 0: {hits / scans:.3f}")
    print(f"  entries needing no scan {ent_none / entries:.3f}; one scan {ent_one / entries:.3f} (of them in the one-obstacle ring as built "
          f"{ent_one_built / entries:.3f}); several {(entries - ent_none - ent_one) / entries:.3f}")
    for k in ("ideal", "built"):
        print(f"  wave-level scans, {k}: {wave['today']} -> {wave[k]} ({wave[k] / wave['today']:.3f}); "
              f"active lanes {lane['today'] / 64 / wave['today']:.3f} -> {lane[k] / 64 / wave[k]:.3f}")


# what profiles/r11_edge/README.md quotes: the benchmark's lattices at both block sizes, and the three obstacle layouts
QUOTED = (("cfg2", 700, 2, "corridor"), ("cfg2", 700, 4, "corridor"), ("cfg5", 48, 4, "corridor"),
          ("cfg2", 252, 2, "survey"), ("cfg2", 252, 2, "worst"))

if __name__ == "__main__":
    a = sys.argv[1:]
    if not a:
        for q in QUOTED:
            price(*q)
    else:
        price(a[0], int(a[1]) if len(a) > 1 else (700 if a[0] == "cfg2" else 48), int(a[2]) if len(a) > 2 else 2,
              a[3] if len(a) > 3 else "corridor")
