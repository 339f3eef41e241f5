"""Writes tests/golden/pcsaft_thermoml.json: 48 molecules of the reference's Esper et al. 2023 PC-SAFT parameter table
(gnnepcsaft/data/esper2023/raw/SI_pcp-saft_parameters.csv), 16 of each class -- non-polar/non-associating, dipolar,
associating -- joined by InChI with ThermoML measurements from gnnepcsaft/data/thermoml/raw/
rho_pure.parquet and vp_pure.parquet (data, not code):

- densities of type "Mass density, kg/m3", phase Liquid, converted to mol/m³ with molweight1;
- vapour pressures with phase_2 Liquid, converted from kPa to Pa, kept between 1 kPa and 2 MPa (away from the triple
  and critical regions, where P_L = P_V cannot be checked tightly in fp64: P_L's absolute rounding is rho_L R T 1e-16);
- at most 8 of each per molecule, spread evenly over the molecule's sorted temperatures.

Each molecule holds its parameter row ``[m, sigma, eps/k, kappa_ab, eps_ab/k, mu, na, nb, mw]`` and its state tables
in the reference's layout ``[T (K), P (Pa), phase, tp, value]`` (tp 1 = density, 3 = vapour pressure; for vapour
pressures P = the measured value).  Molecules are taken in InChI order among those with at least 4 density and 4
vapour-pressure points.  The Esper table has no dipolar+associating molecule (its "opt" column is NONPOLAR, DIPOLAR
or ASSOCIATIVE), so that class is empty here; the GPU tests cover it with random parameter rows.

Run (in the build container, where /root/reference exists):  python tests/golden/make_pcsaft_fixture.py
"""
import csv
import json
import os

import numpy as np
import pandas as pd

REF = "/root/reference/gnnepcsaft/data"
DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pcsaft_thermoml.json")
PER_CLASS, PER_KIND, MIN_POINTS = 16, 8, 4


def _f(s):
    return float(s) if s not in ("", None) else 0.0


def _spread(df, n):
    df = df.sort_values(["T_K", "value"]).drop_duplicates(["T_K"])
    if len(df) <= n:
        return df
    return df.iloc[np.unique(np.round(np.linspace(0, len(df) - 1, n)).astype(int))]


def main():
    rows = list(csv.DictReader(open(os.path.join(REF, "esper2023/raw/SI_pcp-saft_parameters.csv")), delimiter="\t"))
    rho = pd.read_parquet(os.path.join(REF, "thermoml/raw/rho_pure.parquet"))
    rho = rho[(rho.type == "Mass density, kg/m3") & (rho.phase_1 == "Liquid")]
    rho = rho.assign(value=rho.rho * 1000.0 / rho.molweight1, P=rho.P_kPa * 1000.0)
    vp = pd.read_parquet(os.path.join(REF, "thermoml/raw/vp_pure.parquet"))
    vp = vp[vp.phase_2 == "Liquid"]
    vp = vp.assign(value=vp.VP_kPa * 1000.0)
    vp = vp[(vp.value >= 1e3) & (vp.value <= 2e6)]
    rho_by, vp_by = dict(tuple(rho.groupby("inchi1"))), dict(tuple(vp.groupby("inchi1")))

    classes = {"nonpolar": [], "dipolar": [], "associating": []}
    for r in sorted(rows, key=lambda r: r["inchi"]):
        p = [_f(r[k]) for k in ("m", "sigma", "epsilon_k", "kappa_ab", "epsilon_k_ab", "mu", "na", "nb", "molarweight")]
        polar, assoc = p[5] > 0, p[3] > 0 and p[6] * p[7] > 0
        cls = "associating" if assoc else ("dipolar" if polar else "nonpolar")
        if polar and assoc or len(classes[cls]) >= PER_CLASS or r["inchi"] not in rho_by or r["inchi"] not in vp_by:
            continue
        d, v = _spread(rho_by[r["inchi"]], PER_KIND), _spread(vp_by[r["inchi"]], PER_KIND)
        if len(d) < MIN_POINTS or len(v) < MIN_POINTS:
            continue
        classes[cls].append({
            "name": r["common_name"], "inchi": r["inchi"], "class": cls, "params": p,
            "rho": [[float(t), float(pp), 1.0, 1.0, float(x)] for t, pp, x in zip(d.T_K, d.P, d.value)],
            "vp": [[float(t), float(x), 1.0, 3.0, float(x)] for t, x in zip(v.T_K, v.value)],
        })
    mols = [m for c in classes.values() for m in c]
    doc = {"source": "Esper et al. 2023 PC-SAFT parameters (reference gnnepcsaft/data/esper2023/raw) joined with "
                     "ThermoML pure-component liquid densities and vapour pressures (reference "
                     "gnnepcsaft/data/thermoml/raw); written by tests/golden/make_pcsaft_fixture.py",
           "molecules": mols}
    with open(DST, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
    print("wrote", DST, {k: len(v) for k, v in classes.items()}, os.path.getsize(DST), "bytes")


if __name__ == "__main__":
    main()
