"""Runs the six mixture PC-SAFT tensor forms and ``pcsaft.density`` / ``pcsaft.vapor_pressure`` on the
point sets the tests define and saves every output array, so that two builds can be compared byte for byte: the fixture
and the random groups of tests/pcsaft_mix_cases.py, the bubble cases of tests/pcsaft_mix_vle_ref.py, the tie-line and
single-phase points of tests/pcsaft_mix_flash_ref.py, and the invalid-input rows of the four mixture GPU tests.  The
state forms take the density form's own rho (1000 mol/m³ where it found none).  With ``--compare`` it reads two such
files instead and prints the SHA-256 of every array of both with a verdict; exit status 1 if any array differs.

Usage: python tools/pcsaft_mix_dump.py --out FILE.npz
       python tools/pcsaft_mix_dump.py --compare A.npz B.npz [--json FILE.json]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _pool(cases, nc=4):
    """cases (rows, x) as one pool: params [B, 9], comp [M, nc] (-1 = unused), x [M, nc]"""
    params, comp, x = [], np.full((len(cases), nc), -1, dtype=np.int64), np.zeros((len(cases), nc))
    for i, (rows, xi) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        x[i, :len(rows)] = xi
    return np.array(params), comp, x


def dump(path):
    import torch
    from gnnepcsaft_amd import pcsaft
    from tests import pcsaft_mix_cases as C
    from tests import pcsaft_mix_flash_ref as F
    from tests import pcsaft_mix_vle_ref as V
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}

    def put(name, values, keys):
        for k, v in zip(keys, values):
            if v is not None:
                out[f"{name}/{k}"] = v.cpu().numpy()

    def d(*arrays):
        return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]

    def four(name, params, comp, owner, T, P, x, kij=None, eab=None):
        """the density form, both fugacity forms and the state form on one point set"""
        p, c, o, t, pp, xx, k, e = d(params, comp, np.asarray(owner, dtype=np.int64), T, P, x, kij, eab)
        rho, st = pcsaft.mixture_density(p, c, xx, t, pp, o, k, e)
        put(name + "/density", (rho, st), ("rho", "status"))
        put(name + "/ln_phi", pcsaft.mixture_ln_phi(p, c, xx, t, pp, o, k, e, pure=True),
            ("rho", "lnphi", "lnphi_pure", "status"))
        r = torch.where(st == 0, rho, torch.full_like(rho, 1000.0))
        put(name + "/state", pcsaft.mixture_state(p, c, xx, t, r, o, k, e), ("a_res", "p", "dpdrho", "status"))
        put(name + "/ln_phi_state", pcsaft.mixture_ln_phi_state(p, c, xx, t, r, o, k, e), ("lnphi", "Z", "status"))

    def bubble(name, params, comp, owner, T, x, kij=None, eab=None):
        p, c, o, t, xx, k, e = d(params, comp, np.asarray(owner, dtype=np.int64), T, x, kij, eab)
        put(name + "/bubble", pcsaft.mixture_bubble_pressure(p, c, xx, t, o, k, e), ("P", "y", "rho_l", "rho_v", "status"))

    def flash(name, params, comp, owner, T, P, z, kij=None, eab=None):
        p, c, o, t, pp, zz, k, e = d(params, comp, np.asarray(owner, dtype=np.int64), T, P, z, kij, eab)
        put(name + "/flash", pcsaft.mixture_tp_flash(p, c, zz, t, pp, o, k, e),
            ("beta", "x", "y", "rho_l", "rho_v", "status"))

    # the binary fixture, plain and with the k_ij / eab of test_kij_and_eab_are_read_from_the_upper_triangle
    params, comp, owner, T, P, x, _ = C.fixture_points()
    four("fixture", params, comp, owner, T, P, x)
    kij, eab = np.zeros((len(comp), 2, 2)), np.full((len(comp), 2, 2), np.nan)
    kij[:, 0, 1] = kij[:, 1, 0] = 0.03
    eab[-1, 0, 1] = eab[-1, 1, 0] = 2400.0
    four("fixture_kij_eab", params, comp, owner, T, P, x, kij, eab)
    # its invalid-input rows (test_pcsaft_mix_gpu.py, test_pcsaft_mix_phi_gpu.py: test_small_and_invalid_inputs)
    k = 8
    own, xs = owner[:k].copy(), x[:k].copy()
    own[1], own[2] = -1, len(comp)
    xs[3, 0], xs[4], xs[5, 1] = -0.1, 0.0, np.nan
    four("fixture_invalid", params, comp, own, T[:k], P[:k], xs)
    bad_comp = comp.copy()
    bad_comp[owner[6]] = [len(params), 0]
    four("fixture_row_past_B", params, bad_comp, owner[:k], T[:k], P[:k], x[:k])
    four("fixture_no_slot_used", params, np.full_like(comp, -1), owner[:k], T[:k], P[:k], x[:k])
    four("fixture_one_slot", params, np.stack([comp[:, 0], np.full(len(comp), -1)], axis=1), owner[:k], T[:k], P[:k], x[:k])
    bad_T, bad_P = T[:k].copy(), P[:k].copy()
    bad_T[0], bad_T[1], bad_T[2], bad_P[3], bad_P[4], bad_P[5] = np.nan, np.inf, -1.0, np.nan, 0.0, -1e5
    four("fixture_bad_T_P", params, comp, owner[:k], bad_T, bad_P, x[:k])
    # the seeded random mixtures of 1 to 4 slots with their k_ij
    for g in C.recorded()[0]:
        four(f"random_nc{g['nc']}", g["rows"], g["comp"], g["owner"], g["T"], g["P"], g["x"], g["kij"])
    # bubble points: the named and the fixture cases, and the rows of test_no_bubble_point_and_invalid_input
    cases = list(V.NAMED) + V.fixture_cases()
    params, comp, x = _pool([(rows, xi) for _, rows, _, xi in cases])
    T = np.array([c[2] for c in cases], dtype=np.float64)
    bubble("cases", params, comp, np.arange(len(cases)), T, x)
    rows = np.array([V.METHANE, V.BUTANE, V.HEXANE, V.PROPANE], dtype=np.float64)
    comp4 = np.array([[0, -1, -1, -1], [1, 2, -1, -1], [0, 1, 2, -1], [0, 3, 1, 2]], dtype=np.int64)
    xs = np.array([[1.0, 0, 0, 0], [0.5, 0.5, 0, 0], [0.1, 0.3, 0.6, 0], [0.1, 0.2, 0.3, 0.4]])
    T4 = np.array([300.0, 350.0, 320.0, 320.0])
    shuffled = np.random.default_rng(5).integers(0, 4, 257)
    bubble("one_to_four_slots", rows, comp4, shuffled, T4[shuffled], xs[shuffled])
    bad_owner = np.array([1, 1, 1, 4, -1, 1, 1, 1])
    bad_T = np.array([350.0, 350.0, 350.0, 350.0, 350.0, np.nan, np.inf, -1.0])
    bad_x = np.tile(xs[1], (8, 1))
    bad_x[0, 0], bad_x[1, :2], bad_x[2, 1] = -0.5, 0.0, np.nan
    bubble("invalid", rows, comp4, bad_owner, bad_T, bad_x)
    # flash: tie-line feeds, single-phase points, one component; the rows of test_single_phase_and_invalid_input
    tie = F.tie_line_points()
    cases = ([(rows, T, P, z) for _, rows, T, P, z, _, _, _ in tie] + [c[1:] for c in F.single_phase_points()] +
             [([V.METHANE], 300.0, 1e6, [1.0])])
    params, comp, z = _pool([(rows, zi) for rows, _, _, zi in cases])
    T, P = np.array([c[1] for c in cases], dtype=np.float64), np.array([c[2] for c in cases], dtype=np.float64)
    flash("cases", params, comp, np.arange(len(cases)), T, P, z)
    _, _, xl = _pool([(rows, xi) for _, rows, _, _, _, xi, _, _ in tie])
    bubble("tie_line_liquids", params, comp, np.arange(len(tie)), T[:len(tie)], xl)
    n_bad = 13
    bad_owner = np.full(n_bad, 2)
    bad_T, bad_P, bad_z = np.full(n_bad, T[2]), np.full(n_bad, P[2]), np.tile(z[2], (n_bad, 1))
    bad_owner[0], bad_owner[1] = len(cases), -1
    bad_T[2], bad_T[3], bad_T[4], bad_T[5] = np.nan, np.inf, -1.0, 0.0
    bad_P[6], bad_P[7], bad_P[8], bad_P[9] = np.nan, np.inf, 0.0, -1e5
    bad_z[10, 0], bad_z[11, :2], bad_z[12, 1] = -0.5, 0.0, np.nan
    flash("invalid", params, comp, bad_owner, bad_T, bad_P, bad_z)
    # the pure kernels on the ThermoML fixture
    with open(os.path.join(C.GOLDEN, "pcsaft_thermoml.json")) as fh:
        mols = json.load(fh)["molecules"]
    rows = np.array([m["params"] for m in mols], dtype=np.float64)
    rho_pts = np.array([(i, s[0], s[1]) for i, m in enumerate(mols) for s in m["rho"]])
    vp_pts = np.array([(i, s[0]) for i, m in enumerate(mols) for s in m["vp"]])
    p, o, t, pp = d(rows, rho_pts[:, 0].astype(np.int64), rho_pts[:, 1], rho_pts[:, 2])
    put("pure/density", pcsaft.density(p, t, pp, o), ("rho", "status"))
    o, t = d(vp_pts[:, 0].astype(np.int64), vp_pts[:, 1])
    put("pure/vapor_pressure", pcsaft.vapor_pressure(p, t, o), ("psat", "rho_l", "rho_v", "status"))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} arrays, {sum(v.size for v in out.values())} values -> {path}")


def compare(path_a, path_b, json_path):
    a, b = np.load(path_a), np.load(path_b)
    rec, same = {}, sorted(a.files) == sorted(b.files)
    for k in sorted(set(a.files) | set(b.files)):
        ha, hb = [hashlib.sha256(f[k].tobytes()).hexdigest() if k in f.files else None for f in (a, b)]
        equal = ha == hb and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
        rec[k] = {"shape": list(a[k].shape) if k in a.files else None, "sha256": [ha, hb], "equal": equal}
        same = same and equal
        if not equal:
            print("DIFFERS", k, ha, hb)
    print(f"{len(rec)} arrays, every array equal byte for byte: {same}")
    if json_path:
        with open(json_path, "w") as fh:
            json.dump({"files": [os.path.basename(path_a), os.path.basename(path_b)], "all_equal": same, "arrays": rec}, fh,
                      indent=1)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.json))
    if not args.out:
        ap.error("--out FILE.npz or --compare A.npz B.npz")
    dump(args.out)


if __name__ == "__main__":
    main()
