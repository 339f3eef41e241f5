"""Writes tests/golden/pcsaft_binary_thermoml.json: 24 binary systems of the reference's ThermoML table
(gnnepcsaft/data/thermoml/raw/binary.parquet, rows with tp == 1: liquid densities), both components joined by InChI
with the reference's Esper et al. 2023 PC-SAFT parameter table (gnnepcsaft/data/esper2023/raw/
SI_pcp-saft_parameters.csv) -- data, not code, as for tests/golden/make_pcsaft_fixture.py.

- Component classes as in the pure fixture: N non-polar/non-associating, D dipolar, A associating.  Four systems of
  each class pair NN, DN, DD, AN, AD, AA, taken in (InChI 1, InChI 2) order among the systems with at least 8 points;
  ethanol + water is one of the four AA systems (cross-association between unlike species).
- At most 8 points per system, spread evenly over the system's points sorted by (x1, T).
- Per point ``[T (K), P (Pa), x1, x2, rho (mol/m³)]`` with the measured molar density
  ``m * 1000 / (x1 mw1 + x2 mw2)`` (m in kg/m³, the reference's demo/utils_binary.py binary_test).

Run (in the build container, where /root/reference exists):  python tests/golden/make_pcsaft_binary_fixture.py
"""
import csv
import json
import os

import numpy as np
import pandas as pd

REF = "/root/reference/gnnepcsaft/data"
DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pcsaft_binary_thermoml.json")
PER_PAIR, PER_SYSTEM, MIN_POINTS = 4, 8, 8
PAIRS = ("NN", "DN", "DD", "AN", "AD", "AA")
ETHANOL, WATER = "InChI=1S/C2H6O/c1-2-3/h3H,2H2,1H3", "InChI=1S/H2O/h1H2"


def _f(s):
    return float(s) if s not in ("", None) else 0.0


def main():
    table = {}
    for r in csv.DictReader(open(os.path.join(REF, "esper2023/raw/SI_pcp-saft_parameters.csv")), delimiter="\t"):
        p = [_f(r[k]) for k in ("m", "sigma", "epsilon_k", "kappa_ab", "epsilon_k_ab", "mu", "na", "nb", "molarweight")]
        polar, assoc = p[5] > 0, p[3] > 0 and p[6] * p[7] > 0
        if polar and assoc:
            continue
        table[r["inchi"]] = (r["common_name"], "A" if assoc else ("D" if polar else "N"), p)
    df = pd.read_parquet(os.path.join(REF, "thermoml/raw/binary.parquet"))
    df = df[(df.tp == 1) & df.inchi1.isin(table) & df.inchi2.isin(table) & (df.inchi1 != df.inchi2)]
    df = df[(df.mlc1 >= 0) & (df.mlc2 >= 0) & (df.m > 0) & (df.PPa > 0) & (df.TK > 0)]
    groups = {k: g for k, g in df.groupby(["inchi1", "inchi2"]) if len(g) >= MIN_POINTS}

    def system(key):
        (n1, c1, p1), (n2, c2, p2) = table[key[0]], table[key[1]]
        g = groups[key].sort_values(["mlc1", "TK", "PPa", "m"]).drop_duplicates(["mlc1", "TK", "PPa"])
        g = g.iloc[np.unique(np.round(np.linspace(0, len(g) - 1, PER_SYSTEM)).astype(int))]
        pts = [[float(t), float(p), float(x1), float(x2), float(m * 1000.0 / (x1 * p1[8] + x2 * p2[8]))]
               for t, p, x1, x2, m in zip(g.TK, g.PPa, g.mlc1, g.mlc2, g.m)]
        return {"names": [n1, n2], "inchi": list(key), "pair": "".join(sorted(c1 + c2)), "params": [p1, p2],
                "points": pts}

    chosen = {p: [] for p in PAIRS}
    ew = [k for k in groups if set(k) == {ETHANOL, WATER}]
    assert ew, "ethanol + water is not in the table"
    chosen["AA"].append(ew[0])
    for key in sorted(groups):
        pair = "".join(sorted(table[key[0]][1] + table[key[1]][1]))
        if len(chosen[pair]) < PER_PAIR and key not in chosen[pair]:
            chosen[pair].append(key)
    systems = [system(k) for p in PAIRS for k in sorted(chosen[p])]
    doc = {"source": "ThermoML binary liquid densities (reference gnnepcsaft/data/thermoml/raw/binary.parquet, tp == 1) "
                     "joined with Esper et al. 2023 PC-SAFT parameters (reference gnnepcsaft/data/esper2023/raw); "
                     "written by tests/golden/make_pcsaft_binary_fixture.py",
           "systems": systems}
    with open(DST, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
    print("wrote", DST, {p: len(v) for p, v in chosen.items()}, sum(len(s["points"]) for s in systems), "points",
          os.path.getsize(DST), "bytes")
    for s in systems:
        print(s["pair"], s["names"], len(s["points"]))


if __name__ == "__main__":
    main()
