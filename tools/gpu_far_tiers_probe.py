#!/usr/bin/env python3
"""The far-tier decision check's GPU half (tests/test_gpu_far_tiers.py starts it as a subprocess, once per library: a
process binds one library, DNP_LIB).  Builds the clouds of `cases()` - clusters whose box distances sit on either side of
the far thresholds, and "witness" rows that decide a tier - runs every patch launcher on them (dnp_patch_fields_tiled_f32
plain / with interaction partials / with a split tail, dnp_patch_fields_ordered_f32 with a tail, the fp64 tabled and ordered
launches), every output written into a NaN-filled buffer, and saves the slabs and partials to one .npz.  The comparison
with the tier each (patch, tile) should take is the test's, on the host.
    DNP_LIB=tools/bin/libdnp_<variant>.so python tools/gpu_far_tiers_probe.py OUT.npz [SECTION ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILE = 128                      # dnp_patch_tile_rows(): the target rows one wavefront owns (the probe checks it)
FAR_RATIO, FAR_RATIO64 = 8e-3, 6e-4
FAR2_SCALE = 5.0736             # tier-2 threshold = far_d2 * FAR2_SCALE (fp32 only)


def thresholds(eps, f64):
    """(far_d2, tier-2 d2 or None) as the launchers compute them: fp32 rounds both to float."""
    if f64:
        return (eps / FAR_RATIO64) ** (2.0 / 3.0), None
    d2 = np.float32((eps / FAR_RATIO) ** (2.0 / 3.0))
    return float(d2), float(d2 * np.float32(FAR2_SCALE))


def _cluster(rng, n, lo, h):
    """n points in the cube [lo, lo + h]; the first two are its corners, so the box is exactly that cube."""
    p = lo + h * rng.random((n, 3))
    p[0], p[1] = lo, lo + h
    return p


def _cloud(rng, centres, sizes, h, dtype):
    xyz = np.concatenate([_cluster(rng, n, c, h) for c, n in zip(centres, sizes)])
    nrm = rng.standard_normal(xyz.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([xyz, nrm], 1).astype(dtype)


def sweep_case(eps, f64, seed):
    """A hub cluster and 8 clusters along +x whose box gaps to the hub are 0.9, 0.99, 1.01 and 1.1 times each threshold
    distance (fp64: its one threshold, and 2.2 / 2.6 times it); every cluster is one 128-row patch = one target tile."""
    rng = np.random.default_rng(seed)
    far_d2, t2 = thresholds(eps, f64)
    thr = [np.sqrt(far_d2)] + ([np.sqrt(t2)] if t2 else [2.4 * np.sqrt(far_d2)])
    gaps = [f * d for d in thr for f in (0.9, 0.99, 1.01, 1.1)]
    h = 0.02 * thr[0]
    centres = [np.zeros(3)] + [np.array([h + g, 0.0, 0.0]) for g in gaps]
    sizes = [TILE] * len(centres)
    return dict(pts=_cloud(rng, centres, sizes, h, np.float64 if f64 else np.float32), sizes=np.array(sizes), n_free=0,
                eps=eps, f64=f64, split=-3)


# witness rows (see witness_case): 1235 = KT slot 1 of the last lane of the partial last tile, a row in no patch;
# 511 = row 128j + 127 of a full tile; 255 = the last source of patch 0; 883 = the last source of patch 3, in the last
# 128-source run of a patch that the split tail (the last 3 patches of the launch) evaluates as a split item
WITNESS_ROWS = (1235, 511, 255, 883)
_W_SIZES = np.array([256, 128, 200, 300, 128, 164])     # + 60 rows in no patch: N = 1236 = 9 tiles + 84 rows


def witness_case(row, present, f64, seed=5, eps=1e-5):
    """Seven clusters on a line, one per patch plus one for the 60 rows in no patch, adjacent boxes 1.5 threshold
    distances apart (tier 1), the others farther (tier 2).  present: the witness row moves from its own cluster into the
    box of a cluster three steps away, which makes its tile and its patch near that cluster - one point decides."""
    rng = np.random.default_rng(seed)
    far_d2, _ = thresholds(eps, f64)
    d = np.sqrt(far_d2)
    h = 0.05 * d
    centres = [np.array([i * (1.5 * d + h), 0.0, 0.0]) for i in range(len(_W_SIZES) + 1)]
    sizes = list(_W_SIZES) + [60]
    pts = _cloud(rng, centres, sizes, h, np.float64 if f64 else np.float32)
    bounds = np.cumsum([0] + sizes)
    own = int(np.searchsorted(bounds, row, side="right") - 1)
    if present:
        other = own - 3 if own >= 3 else own + 3
        pts[row, :3] = centres[other] + 0.5 * h
    return dict(pts=pts, sizes=_W_SIZES.copy(), n_free=60, eps=eps, f64=f64, split=-3)


def cases():
    out = {}
    # fp32 from just above kNormEps = 2^-48 (below it the fp32 launches run kNorm and no far chain), fp64 from 2e-25
    for i, (e32, e64) in enumerate(((4e-15, 2e-25), (1e-12, 1e-12), (1e-5, 1e-5), (1e-2, 1e-2))):
        out[f"sweep32_{e32:g}"] = sweep_case(e32, False, 100 + i)
        out[f"sweep64_{e64:g}"] = sweep_case(e64, True, 200 + i)
    for row in WITNESS_ROWS:
        for present in (0, 1):
            out[f"witness32_{row}_{present}"] = witness_case(row, present, False)
            out[f"witness64_{row}_{present}"] = witness_case(row, present, True)
    return out


def truncation_case(ratio, scale, f64, eps=1e-5, seed=9, n_tgt=TILE):
    """One source (row 0, a unit dipole; the rest of its 128-row patch are zero dipoles at the same place) and n_tgt
    targets on a cap around +x at |r| = scale * (eps / ratio)^(1/3): e = eps / |r|^3 = ratio / scale^3 for every pair, and the
    only pair a target row has is that one source.  The cap keeps the tile's box off the source's: the forced variants
    run their far chain on it."""
    rng = np.random.default_rng(seed)
    r = scale * (eps / ratio) ** (1.0 / 3.0)
    src = np.zeros((TILE, 6))
    src[:, :3] = 0.25
    src[0, 3:] = rng.standard_normal(3)
    src[0, 3:] /= np.linalg.norm(src[0, 3:])
    v = rng.standard_normal((n_tgt, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[:, 0] = np.abs(v[:, 0]) + 1.0                     # within 60 degrees of +x
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    tgt = np.zeros((n_tgt, 6))
    tgt[:, :3] = 0.25 + r * v
    tgt[:, 3] = 1.0
    pts = np.concatenate([src, tgt]).astype(np.float64 if f64 else np.float32)
    return dict(pts=pts, sizes=np.array([TILE, n_tgt]), n_free=0, eps=eps, f64=f64, split=1)


def truncation_cases():
    out = {}
    for tag, ratio, f64 in (("t32", FAR_RATIO, False), ("t2_32", FAR_RATIO / FAR2_SCALE ** 1.5, False), ("t64", FAR_RATIO64, True)):
        # ten times farther out the truncation is gone: 8 tiles of targets there measure the chain's rounding floor
        for scale, n_tgt in ((1.0, TILE), (10.0, 8 * TILE)):
            out[f"trunc_{tag}_{scale:g}"] = truncation_case(ratio, scale, f64, n_tgt=n_tgt)
    return out


def run(case, dev, torch, fu):
    """Every launch form of the case: {form: slabs [P, N, 3]} and {form + '_wpart': partials}."""
    pts = torch.from_numpy(case["pts"]).to(dev)
    sizes = case["sizes"]
    P, N = len(sizes), pts.shape[0]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
    pp = torch.cat([torch.repeat_interleave(torch.arange(P, device=dev), off[1:] - off[:-1]),
                    torch.full((case["n_free"],), -1, dtype=torch.int64, device=dev)])
    boxes, tiles = fu._patch_boxes(pts, off, None), fu._TileTables(pts, sizes)
    assert tiles.rows == TILE, tiles.rows
    res = {}

    def slabs(name, *args, **kw):
        poisoned = torch.full((P, N, 3), float("nan"), dtype=pts.dtype, device=dev)
        fu._patch_slabs(pts, off, None, pp, 0, P, case["eps"], boxes, tiles.boxes, *args, out=poisoned, **kw)
        res[name] = poisoned.cpu().numpy()

    slabs("tiled", None, 1)
    if tiles.slots:
        wp = torch.full((P, tiles.n_tiles, tiles.slots), float("nan"), dtype=torch.float64, device=dev)
        slabs("tiled_w", wp, 1)
        res["tiled_w_wpart"] = wp.cpu().numpy()
    rev = torch.from_numpy(np.arange(P)[::-1].astype(np.int32).copy()).to(dev)
    if not case["f64"]:
        slabs("tail", None, case["split"])
        slabs("ordered_tail", None, -2, rev)
    else:
        slabs("ordered", None, 1, rev)
    torch.cuda.synchronize()
    return res


def main():
    import torch
    from dipole_normal_prop_amd import _lib
    from dipole_normal_prop_amd import field_utils as fu
    out = sys.argv[1]
    sections = sys.argv[2:] or ["tiers", "truncation"]
    _lib.require_device()
    dev = torch.device("cuda:0")
    all_cases = {}
    if "tiers" in sections:
        all_cases.update(cases())
    if "truncation" in sections:
        all_cases.update(truncation_cases())
    arrays = {}
    for name, case in all_cases.items():
        for form, a in run(case, dev, torch, fu).items():
            arrays[f"{name}/{form}"] = a
    np.savez(out, **arrays)
    print(f"{len(arrays)} arrays from {len(all_cases)} clouds -> {out}")


if __name__ == "__main__":
    main()
