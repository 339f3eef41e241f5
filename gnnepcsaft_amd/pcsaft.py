"""Pure-component PC-SAFT liquid density and vapour pressure on the GPU, for the validation metrics of
``GNNePCSAFTL.validation_step`` (``mape_den`` / ``mape_vp``), with the saturation line's enthalpy and entropy, critical
points and phase diagrams, and PC-SAFT mixtures.

Stands in for the reference's feos calls (gnnepcsaft/train/utils.py:238-300 ``rho_batch`` / ``vp_batch`` and
pcsaft/pcsaft_feos.py ``pure_den_feos`` / ``pure_vp_feos``), with the same arguments and results.  The arithmetic is
the fp64 kernel of csrc/gnx_pcsaft.hip; there is no CPU path.

Enable the native evaluation on a model with::

    from gnnepcsaft_amd import pcsaft
    model.rho_batch, model.vp_batch = pcsaft.rho_batch, pcsaft.vp_batch

The rest of the reference's pure-component entries sit on the same saturation line (csrc/gnx_pcsaft.hip):
``critical_points`` (``critical_points_feos``: ``[Tc (K), Pc (Pa), Dc (mol/m³)]``), ``pure_h_lv`` (``pure_h_lv_feos``,
kJ/mol), ``pure_s_lv`` (``pure_s_lv_feos``, J/mol/K) and ``phase_diagram`` (``phase_diagram_feos``) for one component,
``critical_points_batch`` / ``h_lv_batch`` / ``s_lv_batch`` for every row or every point of every table in one launch,
``saturation`` / ``critical_point`` on device tensors.  Enthalpies and entropies are residual ones, the entropy at the
same T and V: ``pure_s_lv`` is the reference's function taken literally and equals h_lv / T - R ln(rho_L / rho_V), not
h_lv / T.  The critical point is the one of the van der Waals loop that vanishes last as T rises.

Binary (and up to quaternary) mixture densities, the reference's second score (demo/utils_binary.py ``binary_test`` ->
pcsaft/pcsaft_feos.py ``mix_den_feos``), come from the mixture kernels of csrc/gnx_pcsaft_mix.hip:
``mix_den`` for one point, ``mix_rho_batch`` for every point of every system in one launch, ``mixture_density`` /
``mixture_state`` on device tensors.

Fugacity coefficients of a liquid mixture, ln phi_i at (T, P, x), and what the reference builds on them with one feos
state (pcsaft/pcsaft_feos.py): ``mix_ln_fugacity_coefficient``, ``mix_ln_fugacity_coefficient_pure``,
``mix_ln_activity_coefficient``, ``mix_e_gibbs_energy``, ``mix_r_gibbs_energy`` and ``mix_gibbs_energy`` for one point,
``mix_ln_phi_batch`` for every point of every system in one launch, ``mixture_ln_phi`` / ``mixture_ln_phi_state`` on
device tensors (csrc/gnx_pcsaft_mix_phi.hip).  There a component with x = 0 stays in the mixture: its ln phi is the
value at infinite dilution.  x is normalised by its sum, and 0 ln 0 counts as 0 in ``mix_gibbs_energy``.

Bubble points of a mixture, the pressure at which the liquid x starts to boil at T and the vapour y that forms
(csrc/gnx_pcsaft_mix_vle.hip): ``mix_bubble`` for one point (the bubble half of the reference's ``mix_vp_feos``),
``mix_bubble_batch`` for every point of every system in one launch, ``mix_vle_pxy`` for the P-x-y diagram of a binary
(``mix_vle_pxy_diagram_feos``), ``mixture_bubble_pressure`` on device tensors.

Dew points of a mixture, the pressure at which the vapour y starts to condense at T and the liquid x that forms
(csrc/gnx_pcsaft_mix_dew.hip): ``mix_dew`` for one point (the dew half of the reference's ``mix_vp_feos``),
``mix_dew_batch`` for every point of every system in one launch, ``mixture_dew_pressure`` on device tensors, and
``mix_vp``, the reference's ``mix_vp_feos`` itself: (bubble pressure, dew pressure) of one composition.  A vapour can have
more than one dew point (retrograde condensation); the one reported is the one the Raoult's-law start leads to.

Bubble and dew temperatures of a mixture at given pressure (csrc/gnx_pcsaft_mix_tvle.hip): ``mix_bubble_t`` and
``mix_dew_t`` for one point (feos ``PhaseEquilibrium.bubble_point`` / ``dew_point`` at given pressure, with ``t_init`` for
feos's ``tp_init``), ``mix_bubble_t_batch`` / ``mix_dew_t_batch`` for every point of every system in one launch,
``mix_vle_txy`` for the isobaric T-x-y diagram of a binary (the reference's ``mix_vle_diagram_feos``),
``mixture_bubble_temperature`` / ``mixture_dew_temperature`` on device tensors.  Near a critical point of the mixture the
kernel's own start does not reach the pressure and the point reports ``STATUS_NO_CONVERGENCE``; a start temperature
from the caller can still get there.

Isothermal two-phase flashes, the split of a feed z at (T, P) into a liquid x and a vapour y with the vapour mole fraction
beta (csrc/gnx_pcsaft_mix_flash.hip): ``mix_tp_flash`` for one point (the reference's ``mix_tp_flash_feos``),
``mix_tp_flash_batch`` for every point of every system in one launch, ``mix_flash_x1`` for the liquid composition of a
binary at every measured (T, P) over a list of trial feeds in one launch (pcsaft/kij.py ``_pred_x1_worker``),
``mixture_tp_flash`` on device tensors.  A feed without a vapour-liquid split at (T, P) reports ``STATUS_SINGLE_PHASE``;
liquid-liquid splits are not looked for.

Tangent-plane stability of a feed z at (T, P), the test the reference runs on every trial feed before it flashes it
(csrc/gnx_pcsaft_mix_stab.hip): ``mix_is_stable`` for one point (the reference's ``is_stable_feos``),
``mix_stability_batch`` for every point of every system in one launch, ``mixture_stability`` on device tensors.  Each
point runs nc + 2 trial phases as rows of one launch; a negative tangent-plane distance comes back with the composition w
that proves it, also where the split is liquid-liquid and the flash reports none.  No flash is started from w here.

Liquid-liquid flashes, the split of a feed z at (T, P) that starts from the w of the stability test
(csrc/gnx_pcsaft_mix_lle.hip): ``mix_lle`` for one point (the reference's ``mix_lle_feos``), ``mix_lle_diagram`` for the
feed at T .. T + 50 K (``mix_lle_diagram_feos``), ``mix_lle_batch`` for every point of every system in two launches,
``mixture_lle_flash`` on device tensors.  x is the phase of higher molar density, beta the mole fraction of the other
one.  Each phase is in the state the stability test gives it, the one of its liquid and vapour roots with the lower Gibbs
energy, so a split whose lighter phase sits on a vapour root is returned as it is: the same tie line ``mix_tp_flash``
finds.  A stable feed reports ``STATUS_SINGLE_PHASE``.  Three-phase (VLLE) states are not looked for.

The k_ij fit of binaries to measured liquid compositions (csrc/gnx_pcsaft_kij.hip; the reference's pcsaft/kij.py):
``optimize_kij`` for a VLE table (the reference's ``optimize_kij``), ``fit_kij`` for the fit alone, every binary in
lockstep with two launches and one small download per Levenberg-Marquardt iteration, ``mix_kij_x1`` for the predicted
x_1 and residuals of one binary under several k_12 in one launch.  Vapour-liquid data only.

Parameter rows are ``[m, sigma (Å), epsilon/k (K), kappa_ab, epsilon_ab/k (K), mu (D), na, nb, mw]``; state rows are
``[T (K), P (Pa), phase, tp, value]`` (only T and P are read).  Densities are in mol/m³, pressures in Pa.
"""
from __future__ import annotations

from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

STATUS_OK, STATUS_NO_CONVERGENCE, STATUS_SUPERCRITICAL, STATUS_BAD_INPUT, STATUS_SINGLE_PHASE = 0, 1, 2, 3, 4
_REASON = {STATUS_NO_CONVERGENCE: "no root / not converged", STATUS_SUPERCRITICAL: "temperature at or above the "
           "critical temperature", STATUS_BAD_INPUT: "invalid parameters or state",
           STATUS_SINGLE_PHASE: "single phase: no vapour-liquid split at this temperature, pressure and feed"}


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.GnxError(_lib.GNX_E_INVALID, "gnnepcsaft_amd.pcsaft needs a HIP device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _upload(dev: torch.device, arrays: Sequence[Optional[np.ndarray]]) -> List[Optional[torch.Tensor]]:
    """Host fp64 / int64 arrays packed into one 8-byte-element buffer and copied once: a device view of each, of its
    shape and in order (None stays None)."""
    given = [a for a in arrays if a is not None]
    ends = np.cumsum([a.size for a in given])
    buf = np.empty(int(ends[-1]), dtype=np.int64)
    flt = buf.view(np.float64)
    for a, end in zip(given, ends):
        (flt if a.dtype == np.float64 else buf)[end - a.size:end] = a.reshape(-1)
    dbuf = torch.from_numpy(buf).to(dev)
    dflt = dbuf.view(torch.float64)
    views = iter([(dflt if a.dtype == np.float64 else dbuf)[end - a.size:end].view(a.shape)
                  for a, end in zip(given, ends)])
    return [None if a is None else next(views) for a in arrays]


def _run_packed(entry, inputs: Sequence[Optional[np.ndarray]], n: int, shapes: Sequence[Optional[Tuple[int, ...]]],
                ints: int = 1, **kw) -> Tuple[List[Optional[np.ndarray]], List[np.ndarray]]:
    """One upload, one launch, one download for host arrays.  ``entry`` is a call site of gnnepcsaft_amd.ops that takes
    ``out``, ``inputs`` its arguments in order, ``shapes`` the shape of each of its fp64 outputs (None: not asked for),
    ``ints`` the number of int32 [n] outputs that follow them in ``out``.  Every output lives in one buffer, the fp64 ones
    followed by the int32 ones (each padded to 8 bytes) -> ([fp64 arrays], [int32 arrays [n]])."""
    dev = _device()
    sizes = [0 if s is None else int(np.prod(s)) for s in shapes]
    ends = np.cumsum(sizes)
    end, half = int(ends[-1]), (n + 1) // 2
    out = torch.empty(end + ints * half, dtype=torch.int64, device=dev)
    flt = out.view(torch.float64)
    views = [None if s is None else flt[e - k:e].view(s) for s, k, e in zip(shapes, sizes, ends)]
    tails = [out[end + j * half:end + (j + 1) * half].view(torch.int32)[:n] for j in range(ints)]
    entry(*_upload(dev, inputs), out=(*views, *tails), **kw)
    host = out.cpu().numpy()
    val = host[:end].view(np.float64)
    return ([None if s is None else val[e - k:e].reshape(s).copy() for s, k, e in zip(shapes, sizes, ends)],
            [host[end + j * half:end + (j + 1) * half].view(np.int32)[:n].copy() for j in range(ints)])


def _run(entry, inputs: Sequence[Optional[np.ndarray]], n: int, shapes: Sequence[Optional[Tuple[int, ...]]], **kw
         ) -> Tuple[List[Optional[np.ndarray]], np.ndarray]:
    """``_run_packed`` for an entry whose one int32 output is the status -> ([fp64 arrays], status [n])."""
    values, (status,) = _run_packed(entry, inputs, n, shapes, **kw)
    return values, status


def _run_pure(kind: str, params: np.ndarray, owner: np.ndarray, T: np.ndarray, P: Optional[np.ndarray]
              ) -> Tuple[np.ndarray, np.ndarray]:
    """(liquid density, kind "rho", or vapour pressure, kind "vp", [n] fp64; status [n] int32)"""
    n = owner.shape[0]
    if kind == "rho":
        values, status = _run(ops._pcsaft_density, [params, owner, T, P], n, [(n,)])
    else:
        values, status = _run(ops._pcsaft_vapor_pressure, [params, owner, T], n, [(n,), None, None])
    return values[0], status


def _rows(parameters_batch: Sequence[Sequence[float]]) -> np.ndarray:
    params = np.asarray(parameters_batch, dtype=np.float64).reshape(-1, 9)
    if params.shape[0] != len(parameters_batch):
        raise ValueError(f"expected {len(parameters_batch)} parameter rows of 9 values, got {np.shape(parameters_batch)}")
    return params


def _nonempty(what: str, count: int, states_batch: List[Any]) -> List[Tuple[int, Any]]:
    """(i, table) of the state tables with rows, after the length check of a batch form"""
    if count != len(states_batch):
        raise ValueError(f"{count} {what} but {len(states_batch)} state tables")
    return [(i, s) for i, s in enumerate(states_batch) if np.shape(s)[0] > 0]


def _run_tables(index: Sequence[int], states: Sequence[np.ndarray], run) -> List[np.ndarray]:
    """states[k]: the [rows, ...] fp64 states of table index[k].  All of them stacked go through ``run(owner, states)``
    -> [n, ...] once, owner being the table of each row; the result comes back split at the table cuts (views)."""
    owner = np.concatenate([np.full(t.shape[0], i, dtype=np.int64) for i, t in zip(index, states)])
    value = run(owner, np.concatenate(states))
    return np.split(value, np.cumsum([t.shape[0] for t in states])[:-1])


def _batch(kind: str, parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    tables = _nonempty("parameter rows", len(parameters_batch), states_batch)
    if not tables:
        return []
    params = _rows(parameters_batch)
    states = [np.asarray(s, dtype=np.float64).reshape(np.shape(s)[0], -1) for _, s in tables]

    def run(owner, st):
        return _run_pure(kind, params, owner, st[:, 0], st[:, 1] if kind == "rho" else None)[0]

    return [v.copy() for v in _run_tables([i for i, _ in tables], states, run)]


def rho_batch(parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    """Liquid densities (mol/m³) of every state of every non-empty table, one fp64 array per such table, 0.0 where a
    point failed (reference train/utils.py:252-268)."""
    return _batch("rho", parameters_batch, states_batch)


def vp_batch(parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    """Vapour pressures (Pa) at the temperature of every state of every non-empty table, one fp64 array per such
    table, 0.0 where a point failed (reference train/utils.py:284-300)."""
    return _batch("vp", parameters_batch, states_batch)


def _require_ok(status: np.ndarray, what: str, state: Sequence[float]) -> None:
    if status[0] != STATUS_OK:
        raise RuntimeError(f"PC-SAFT {what} failed at state {list(state)}: {_REASON.get(int(status[0]), int(status[0]))}")


def _single(kind: str, parameters: Sequence[float], state: Sequence[float]) -> float:
    params = _rows([parameters])
    P = np.asarray([state[1]], dtype=np.float64) if kind == "rho" else None
    value, status = _run_pure(kind, params, np.zeros(1, dtype=np.int64), np.asarray([state[0]], dtype=np.float64), P)
    _require_ok(status, "density" if kind == "rho" else "vapor pressure", state)
    return float(value[0])


def pure_den(parameters: Sequence[float], state: Sequence[float]) -> float:
    """Liquid density (mol/m³) at ``state = [T (K), P (Pa), ...]`` (reference ``pure_den_feos``); raises
    ``RuntimeError`` where no liquid root is found."""
    return _single("rho", parameters, state)


def pure_vp(parameters: Sequence[float], state: Sequence[float]) -> float:
    """Vapour pressure (Pa) at ``state = [T (K), ...]`` (reference ``pure_vp_feos``); raises ``RuntimeError`` at or
    above the critical temperature and where the phase equilibrium does not converge."""
    return _single("vp", parameters, state)


def _owner(owner: Optional[torch.Tensor], T: torch.Tensor) -> torch.Tensor:
    if owner is not None:
        return owner
    return torch.arange(T.numel(), dtype=torch.int64, device=T.device)


def density(params: torch.Tensor, T: torch.Tensor, P: torch.Tensor, owner: Optional[torch.Tensor] = None
            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors: params [B, 9] fp64, T / P [n] fp64, owner [n] int64 (default: point i uses row
    i) -> (rho [n] mol/m³, status [n] int32).  Asynchronous, on the current stream."""
    return ops.pcsaft_density(params, _owner(owner, T), T, P)


def vapor_pressure(params: torch.Tensor, T: torch.Tensor, owner: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors: params [B, 9] fp64, T [n] fp64, owner [n] int64 (default: point i uses row i)
    -> (psat [n] Pa, rho_l [n], rho_v [n] mol/m³, status [n] int32).  Asynchronous, on the current stream."""
    return ops.pcsaft_vapor_pressure(params, _owner(owner, T), T)


# ---- the saturation line and the critical point of a pure component ---------------------------------
def saturation(params: torch.Tensor, T: torch.Tensor, owner: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
    """Tensor form on device tensors: params [B, 9] fp64, T [n] fp64, owner [n] int64 (default: point i uses row i)
    -> (psat [n] Pa, rho_l [n], rho_v [n] mol/m³, h_l [n], h_v [n] J/mol, s_l [n], s_v [n] J/mol/K, status [n] int32).
    h = R T (-T a_T + Z - 1) and s = -R (a + T a_T) are the residual molar enthalpy and the residual molar entropy at the
    same T and V.  Asynchronous, on the current stream."""
    return ops.pcsaft_saturation(params, _owner(owner, T), T)


def critical_point(params: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors: params [B, 9] fp64 -> (Tc [B] K, Pc [B] Pa, rho_c [B] mol/m³, status [B] int32),
    the vapour-liquid critical point of every row.  Asynchronous, on the current stream."""
    return ops.pcsaft_critical_point(params)


def _run_saturation(params: np.ndarray, owner: np.ndarray, T: np.ndarray) -> Tuple[List[np.ndarray], np.ndarray]:
    """([psat, rho_l, rho_v, h_l, h_v, s_l, s_v] [n] fp64, status [n] int32)"""
    n = owner.shape[0]
    return _run(ops._pcsaft_saturation, [params, owner, T], n, [(n,)] * 7)


def _run_critical(params: np.ndarray, with_h_s: bool = False) -> Tuple[List[Optional[np.ndarray]], np.ndarray]:
    """([Tc, Pc, rho_c, h_c, s_c] [B] fp64, the last two None unless asked for; status [B] int32)"""
    B = params.shape[0]
    return _run(ops._pcsaft_critical_point, [params], B, [(B,)] * 3 + [(B,) if with_h_s else None] * 2)


def critical_points(parameters: Sequence[float]) -> List[float]:
    """Vapour-liquid critical point ``[Tc (K), Pc (Pa), Dc (mol/m³)]`` of a pure component (reference
    ``critical_points_feos``): the state with (dp/drho)_T = (d²p/drho²)_T = 0 on the van der Waals loop that vanishes last
    as T rises.  Raises ``RuntimeError`` where it is not found."""
    (Tc, Pc, Dc, _, _), status = _run_critical(_rows([parameters]))
    _require_ok(status, "critical point", [])
    return [float(Tc[0]), float(Pc[0]), float(Dc[0])]


def critical_points_batch(parameters_batch: Sequence[Sequence[float]]) -> np.ndarray:
    """``[Tc (K), Pc (Pa), Dc (mol/m³)]`` of every parameter row as a [B, 3] array in one launch, rows of 0.0 where a row
    failed."""
    if len(parameters_batch) == 0:
        return np.zeros((0, 3), dtype=np.float64)
    (Tc, Pc, Dc, _, _), _ = _run_critical(_rows(parameters_batch))
    return np.stack([Tc, Pc, Dc], axis=1)


def _lv(kind: str, values: List[np.ndarray]) -> np.ndarray:
    """h_lv in kJ/mol (kind "h") or s_lv in J/mol/K (kind "s") from the outputs of the saturation entry"""
    return (values[4] - values[3]) / 1e3 if kind == "h" else values[6] - values[5]


def _single_lv(kind: str, parameters: Sequence[float], state: Sequence[float]) -> float:
    values, status = _run_saturation(_rows([parameters]), np.zeros(1, dtype=np.int64),
                                     np.asarray([state[0]], dtype=np.float64))
    _require_ok(status, "enthalpy of vaporization" if kind == "h" else "entropy of vaporization", state)
    return float(_lv(kind, values)[0])


def pure_h_lv(parameters: Sequence[float], state: Sequence[float]) -> float:
    """Enthalpy of vaporization h_V - h_L (kJ/mol) at ``state = [T (K), ...]`` (reference ``pure_h_lv_feos``).  The
    ideal-gas part depends on T only, so the difference of the residual enthalpies is the full one.  Raises
    ``RuntimeError`` at or above the critical temperature and where the phase equilibrium does not converge."""
    return _single_lv("h", parameters, state)


def pure_s_lv(parameters: Sequence[float], state: Sequence[float]) -> float:
    """Difference s_V - s_L of the residual molar entropies (J/mol/K) at ``state = [T (K), ...]``: the reference's
    ``pure_s_lv_feos`` taken literally.  The residual is the one at the same T and V (what feos's
    ``Contributions.Residual`` means, as far as that can be told without feos), so this is **not** h_lv / T: at saturation
    s_lv = h_lv / T - R ln(rho_L / rho_V), and the full entropy of vaporization is h_lv / T.  Raises ``RuntimeError`` as
    ``pure_h_lv`` does."""
    return _single_lv("s", parameters, state)


def _lv_batch(kind: str, parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    tables = _nonempty("parameter rows", len(parameters_batch), states_batch)
    if not tables:
        return []
    params = _rows(parameters_batch)
    states = [np.asarray(s, dtype=np.float64).reshape(np.shape(s)[0], -1) for _, s in tables]

    def run(owner, st):
        return _lv(kind, _run_saturation(params, owner, np.ascontiguousarray(st[:, 0]))[0])

    return [v.copy() for v in _run_tables([i for i, _ in tables], states, run)]


def h_lv_batch(parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    """Enthalpies of vaporization (kJ/mol) at the temperature of every state of every non-empty table, one fp64 array per
    such table, 0.0 where a point failed: ``vp_batch``'s form, one launch."""
    return _lv_batch("h", parameters_batch, states_batch)


def s_lv_batch(parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    """``pure_s_lv`` (J/mol/K) at the temperature of every state of every non-empty table, one fp64 array per such table,
    0.0 where a point failed: ``vp_batch``'s form, one launch."""
    return _lv_batch("s", parameters_batch, states_batch)


PHASE_DIAGRAM_KEYS = ("temperature", "pressure", "density liquid", "density vapor", "mass density liquid",
                      "mass density vapor", "molar enthalpy liquid", "molar enthalpy vapor", "molar entropy liquid",
                      "molar entropy vapor", "specific enthalpy liquid", "specific enthalpy vapor",
                      "specific entropy liquid", "specific entropy vapor")


def phase_diagram(parameters: Sequence[float], state: Sequence[float], points: int = 200) -> dict:
    """Phase diagram of a pure component from ``state[0]`` (K) to the critical point (reference ``phase_diagram_feos``;
    feos ``PhaseDiagram.pure(eos, T, points).to_dict(Contributions.Residual)``) as a dict of equally long lists under
    ``PHASE_DIAGRAM_KEYS``: ``temperature`` (K), ``pressure`` (Pa), ``density liquid`` / ``density vapor`` (mol/m³),
    ``mass density ...`` (kg/m³, from mw in g/mol), ``molar enthalpy ...`` (kJ/mol), ``molar entropy ...`` (kJ/mol/K),
    ``specific enthalpy ...`` (kJ/kg), ``specific entropy ...`` (kJ/kg/K); enthalpies and entropies are the residual ones
    of ``saturation``.  Tc comes from the critical-point launch, then one saturation launch runs at
    linspace(state[0], Tc, points)[:-1]; the last entry is the critical point itself, both phases at rho_c.  Points whose
    status is not 0 are dropped.  ``ValueError`` if ``state[0] >= Tc``, if the critical point is not found, or if nothing
    is left.  The key spelling and the placement of the points have not been checked against feos's ``to_dict``."""
    if int(points) < 2:
        raise ValueError(f"a phase diagram needs at least 2 points, got {points}")
    params = _rows([parameters])
    (Tc, Pc, Dc, hc, sc), cstatus = _run_critical(params, with_h_s=True)
    if cstatus[0] != STATUS_OK:
        raise ValueError(f"no critical point found: {_REASON.get(int(cstatus[0]), int(cstatus[0]))}")
    t0 = float(state[0])
    if not t0 < Tc[0]:
        raise ValueError(f"the start temperature {t0} K is not below the critical temperature {float(Tc[0])} K")
    T = np.linspace(t0, float(Tc[0]), int(points))[:-1]
    values, status = _run_saturation(params, np.zeros(T.shape[0], dtype=np.int64), T)
    keep = status == STATUS_OK
    if not keep.any():
        raise ValueError("No VLE found at the given conditions.")
    P, rl, rv, hl, hv, sl, sv = (v[keep] for v in values)
    T = np.append(T[keep], Tc[0])
    P = np.append(P, Pc[0])
    rl, rv = np.append(rl, Dc[0]), np.append(rv, Dc[0])
    hl, hv = np.append(hl, hc[0]) / 1e3, np.append(hv, hc[0]) / 1e3      # kJ/mol
    sl, sv = np.append(sl, sc[0]) / 1e3, np.append(sv, sc[0]) / 1e3      # kJ/mol/K
    mw = float(params[0, 8]) / 1e3                                       # kg/mol
    columns = (T, P, rl, rv, rl * mw, rv * mw, hl, hv, sl, sv, hl / mw, hv / mw, sl / mw, sv / mw)
    return {key: col.tolist() for key, col in zip(PHASE_DIAGRAM_KEYS, columns)}


# ---- mixtures of 1 to 4 components (csrc/gnx_pcsaft_mix.hip) ------------------------------------------
NC_MAX = 4


def mixture_state(params: torch.Tensor, comp: torch.Tensor, x: torch.Tensor, T: torch.Tensor, rho: torch.Tensor,
                  owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                  eab: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors: params [B, 9] fp64 pool of component rows, comp [M, nc] int64 rows of each
    mixture (-1 = unused slot), x [n, nc] fp64 compositions (normalised by their sum), T [n] K, rho [n] mol/m³, owner [n]
    int64 mixture of each point (default: point i is mixture i), kij / eab [M, nc, nc] fp64 (upper triangle read; NaN
    in eab = combining rule) -> (a_res [n], p [n] Pa, dpdrho [n] Pa·m³/mol, status [n] int32).  Asynchronous, on the
    current stream."""
    return ops.pcsaft_mix_state(params, comp, kij, eab, _owner(owner, T), T, rho, x)


def mixture_density(params: torch.Tensor, comp: torch.Tensor, x: torch.Tensor, T: torch.Tensor, P: torch.Tensor,
                    owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                    eab: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_state`` with P [n] Pa in place of rho -> (rho [n] mol/m³,
    status [n] int32).  Asynchronous, on the current stream."""
    return ops.pcsaft_mix_density(params, comp, kij, eab, _owner(owner, T), T, P, x)


def mixture_ln_phi_state(params: torch.Tensor, comp: torch.Tensor, x: torch.Tensor, T: torch.Tensor, rho: torch.Tensor,
                         owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                         eab: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_state`` -> (lnphi [n, nc], Z [n], status [n] int32): the
    fugacity coefficients ln phi_i and the compressibility factor at the molar density rho.  NaN in a -1 slot and in the
    whole row where status != 0; a used slot with x = 0 reports its infinite-dilution value.  Asynchronous, on the
    current stream."""
    return ops.pcsaft_mix_lnphi_state(params, comp, kij, eab, _owner(owner, T), T, rho, x)


def mixture_ln_phi(params: torch.Tensor, comp: torch.Tensor, x: torch.Tensor, T: torch.Tensor, P: torch.Tensor,
                   owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                   eab: Optional[torch.Tensor] = None, pure: bool = False
                   ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_density`` -> (rho [n] mol/m³, lnphi [n, nc], lnphi_pure
    [n, nc] or None, status [n] int32): the liquid root of ``mixture_density`` (the same bits), ln phi_i there and, with
    ``pure``, ln phi of each component alone at its own liquid root at the same T and P (NaN where it has none; the
    status stays 0).  Asynchronous, on the current stream."""
    return ops.pcsaft_mix_lnphi(params, comp, kij, eab, _owner(owner, T), T, P, x, pure)


def mixture_bubble_pressure(params: torch.Tensor, comp: torch.Tensor, x: torch.Tensor, T: torch.Tensor,
                            owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                            eab: Optional[torch.Tensor] = None
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_state`` without rho -> (P [n] Pa, y [n, nc], rho_l [n],
    rho_v [n] mol/m³, status [n] int32): the bubble point of the liquid x at T.  A used slot with x = 0 is dropped
    (y = 0.0), a -1 slot has y = NaN; where status != 0 (1 also means "no bubble point at this T"), P and the densities
    are 0.0 and the y row is NaN.  Asynchronous, on the current stream."""
    return ops.pcsaft_mix_bubble(params, comp, kij, eab, _owner(owner, T), T, x)


def mixture_dew_pressure(params: torch.Tensor, comp: torch.Tensor, y: torch.Tensor, T: torch.Tensor,
                         owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                         eab: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_bubble_pressure`` with the vapour y [n, nc] in place of x ->
    (P [n] Pa, x [n, nc], rho_l [n], rho_v [n] mol/m³, status [n] int32): the dew point of the vapour y at T.  A used slot
    with y = 0 is dropped (x = 0.0), a -1 slot has x = NaN; where status != 0 (1 also means "no dew point found at this
    T"), P and the densities are 0.0 and the x row is NaN.  Asynchronous, on the current stream."""
    return ops.pcsaft_mix_dew(params, comp, kij, eab, _owner(owner, T), T, y)


def mixture_bubble_temperature(params: torch.Tensor, comp: torch.Tensor, x: torch.Tensor, P: torch.Tensor,
                               owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                               eab: Optional[torch.Tensor] = None, T0: Optional[torch.Tensor] = None
                               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_bubble_pressure`` with P [n] Pa in place of T -> (T [n] K,
    y [n, nc], rho_l [n], rho_v [n] mol/m³, status [n] int32): the temperature at which the liquid x starts to boil at P.
    T0 [n] or None: the temperature each solve starts from, NaN for the kernel's own start.  A used slot with x = 0 is
    dropped (y = 0.0), a -1 slot has y = NaN; where status != 0 (1: no bubble temperature found, 3: bad input, a
    P <= 0 or a T0 <= 0 included), T and the densities are 0.0 and the y row is NaN.  Asynchronous, on the current
    stream."""
    return ops.pcsaft_mix_bubble_t(params, comp, kij, eab, _owner(owner, P), P, x, T0)


def mixture_dew_temperature(params: torch.Tensor, comp: torch.Tensor, y: torch.Tensor, P: torch.Tensor,
                            owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                            eab: Optional[torch.Tensor] = None, T0: Optional[torch.Tensor] = None
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_bubble_temperature`` with the vapour y [n, nc] in place of
    x -> (T [n] K, x [n, nc], rho_l [n], rho_v [n] mol/m³, status [n] int32): the temperature at which the vapour y
    starts to condense at P.  A used slot with y = 0 is dropped (x = 0.0), a -1 slot has x = NaN; where status != 0, T
    and the densities are 0.0 and the x row is NaN.  Asynchronous, on the current stream."""
    return ops.pcsaft_mix_dew_t(params, comp, kij, eab, _owner(owner, P), P, y, T0)


def mixture_tp_flash(params: torch.Tensor, comp: torch.Tensor, z: torch.Tensor, T: torch.Tensor, P: torch.Tensor,
                     owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                     eab: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_density`` with the feed z [n, nc] in place of x -> (beta [n],
    x [n, nc], y [n, nc], rho_l [n], rho_v [n] mol/m³, status [n] int32): the split of z at (T, P) into the liquid x and the
    vapour y, beta the vapour mole fraction, z = (1 - beta) x + beta y.  A used slot with z = 0 is dropped (x = y = 0.0), a
    -1 slot has NaN; where status != 0 (4 = ``STATUS_SINGLE_PHASE``: no vapour-liquid split), beta and the densities are
    0.0 and the x and y rows are NaN.  Asynchronous, on the current stream."""
    return ops.pcsaft_mix_flash(params, comp, kij, eab, _owner(owner, T), T, P, z)


def _reduce_trials(tpd: torch.Tensor, w: torch.Tensor, status: torch.Tensor
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The verdict of each point from its trials, tpd / status [n, nt] and w [n, nt, nc] of ``ops.pcsaft_mix_stability``
    -> (stable [n] bool, tpd [n], w [n, nc], status [n] int32).  A trial with status 0 and tpd < 0 makes the point
    unstable with status 0, whatever the other trials did: it gets the most negative tpd and its w.  Otherwise a trial
    status != 0 is the point's (3 over 1): not stable, tpd and w NaN.  Otherwise the point is stable: the smallest
    stationary tpd and its w, or 0.0 and the feed (trial 0) where every trial fell onto the feed (tpd = 0.0 exactly)."""
    ok = status == STATUS_OK
    unstable = (ok & (tpd < 0)).any(dim=1)
    st = torch.where(unstable, torch.zeros_like(status[:, 0]), status.max(dim=1).values)
    pick = torch.where(ok & (tpd != 0), tpd, torch.full_like(tpd, float("inf"))).argmin(dim=1)
    point = torch.arange(tpd.size(0), device=tpd.device)
    lost = (st != STATUS_OK)
    nan = torch.full_like(tpd[:, 0], float("nan"))
    return (~unstable & ~lost, torch.where(lost, nan, tpd[point, pick]),
            torch.where(lost[:, None], nan[:, None], w[point, pick]), st)


def mixture_stability(params: torch.Tensor, comp: torch.Tensor, z: torch.Tensor, T: torch.Tensor, P: torch.Tensor,
                      owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                      eab: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_tp_flash`` -> (stable [n] bool, tpd [n], w [n, nc], status [n]
    int32): Michelsen's tangent-plane test of the feed z at (T, P).  Each point becomes nc + 2 rows of one launch of
    ``ops.pcsaft_mix_stability`` (trial 0 vapour-like, 1 liquid-like, 2 + s rich in slot s), reduced on the device as
    ``_reduce_trials`` says: unstable with the most negative tangent-plane distance tpd and the composition w that has
    it; stable with the smallest stationary tpd (0.0 and w = z where every trial fell onto the feed); or, with status
    != 0, neither: ``stable`` False, tpd and w NaN.  In w a used slot with z = 0 has 0.0, a -1 slot NaN.  Asynchronous, on
    the current stream."""
    n, nc = z.shape
    nt = nc + 2
    trial = torch.arange(nt, dtype=torch.int64, device=z.device).repeat(n)
    tpd, w, _, _, status = ops.pcsaft_mix_stability(
        params, comp, kij, eab, _owner(owner, T).repeat_interleave(nt), trial, T.repeat_interleave(nt),
        P.repeat_interleave(nt), z.repeat_interleave(nt, dim=0))
    return _reduce_trials(tpd.view(n, nt), w.view(n, nt, nc), status.view(n, nt))


def mixture_lle_flash(params: torch.Tensor, comp: torch.Tensor, z: torch.Tensor, T: torch.Tensor, P: torch.Tensor,
                      owner: Optional[torch.Tensor] = None, kij: Optional[torch.Tensor] = None,
                      eab: Optional[torch.Tensor] = None, w0: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tensor form on device tensors, arguments as ``mixture_tp_flash`` -> (beta [n], x [n, nc], y [n, nc], rho_x [n],
    rho_y [n] mol/m³, status [n] int32): the split of z at (T, P) into two phases, x the one of higher molar density, beta
    the mole fraction of the other one, z = (1 - beta) x + beta y.  w0 [n, nc]: the composition the second phase starts
    from, one launch of ``ops.pcsaft_mix_lle``.  Without it ``mixture_stability`` runs first and the split starts from
    its w: a stable feed ends at once with status 4 (``STATUS_SINGLE_PHASE``), and where the stability test is
    inconclusive its status is the point's.  A used slot with z = 0 is dropped (x = y = 0.0), a -1 slot has NaN; where
    status != 0, beta and the densities are 0.0 and the x and y rows are NaN.  Asynchronous, on the current stream."""
    owner = _owner(owner, T)
    if w0 is not None:
        return ops.pcsaft_mix_lle(params, comp, kij, eab, owner, T, P, z, w0)
    _, tpd, w, st = mixture_stability(params, comp, z, T, P, owner, kij, eab)
    # w only where it proves the feed unstable; the feed itself (no split: status 4, or the feed's own status 3) elsewhere
    out = ops.pcsaft_mix_lle(params, comp, kij, eab, owner, T, P, z, torch.where((tpd < 0)[:, None], w, z))
    return (*out[:5], torch.where(st != STATUS_OK, st, out[5]))


def _run_mix(kind: str, params: np.ndarray, comp: np.ndarray, kij: Optional[np.ndarray], eab: Optional[np.ndarray],
             owner: np.ndarray, states: np.ndarray, start: Optional[np.ndarray] = None
             ) -> Tuple[List[Optional[np.ndarray]], np.ndarray]:
    """states [n, 2 + nc] -> (values, status [n] int32); values is [rho [n]] for kind "density", [rho, lnphi [n, nc],
    None] for "lnphi", [rho, lnphi, lnphi_pure [n, nc]] for "lnphi_pure" and [P [n], y [n, nc], rho_l [n], rho_v [n]]
    for "bubble", which does not read the P column, [P [n], x [n, nc], rho_l [n], rho_v [n]] for "dew", whose composition
    columns hold the vapour and which does not read it either, and [beta [n], x [n, nc], y [n, nc], rho_l [n], rho_v [n]]
    for "flash", whose composition columns hold the feed, as do those of "stability": [tpd [n], w [n, nc]] of the points,
    their nc + 2 trials each expanded here into rows of the launch and reduced by ``_reduce_trials`` after the
    download.  "lle" is "stability" and then the liquid-liquid entry started from its w, two launches: [beta [n], x
    [n, nc], y [n, nc], rho_x [n], rho_y [n]].  "bubble_t" and "dew_t" are "bubble" and "dew" at given pressure: they
    read the P column and not the T column, values is [T [n], y or x [n, nc], rho_l [n], rho_v [n]], and ``start`` [n] (theirs alone) holds the
    temperatures the solves start from, NaN or no array at all for the kernel's own start."""
    n, nc = owner.shape[0], comp.shape[1]
    if kind in ("bubble_t", "dew_t"):
        entry = ops._pcsaft_mix_bubble_t if kind == "bubble_t" else ops._pcsaft_mix_dew_t
        return _run(entry, [params, comp, kij, eab, owner, states[:, 1], states[:, 2:], start], n,
                    [(n,), (n, nc), (n,), (n,)])
    if kind == "stability":
        nt = nc + 2
        rows = [np.repeat(a, nt, axis=0) for a in (owner, states[:, 0], states[:, 1], states[:, 2:])]
        trial = np.tile(np.arange(nt, dtype=np.int64), n)
        (tpd, w, _, _), status = _run(ops._pcsaft_mix_stability, [params, comp, kij, eab, rows[0], trial, *rows[1:]],
                                      n * nt, [(n * nt,), (n * nt, nc), None, None])
        _, tpd, w, status = _reduce_trials(torch.from_numpy(tpd).view(n, nt), torch.from_numpy(w).view(n, nt, nc),
                                           torch.from_numpy(status).view(n, nt))
        return [tpd.numpy(), w.numpy()], status.numpy()
    if kind == "lle":
        (tpd, w), st = _run_mix("stability", params, comp, kij, eab, owner, states)
        first = np.where((tpd < 0)[:, None], w, states[:, 2:])  # as ``mixture_lle_flash`` starts it
        values, status = _run(ops._pcsaft_mix_lle, [params, comp, kij, eab, owner, states[:, 0], states[:, 1],
                                                    states[:, 2:], first], n, [(n,), (n, nc), (n, nc), (n,), (n,)])
        return values, np.where(st != STATUS_OK, st, status)
    if kind == "flash":
        return _run(ops._pcsaft_mix_flash, [params, comp, kij, eab, owner, states[:, 0], states[:, 1], states[:, 2:]], n,
                    [(n,), (n, nc), (n, nc), (n,), (n,)])
    if kind in ("bubble", "dew"):
        entry = ops._pcsaft_mix_bubble if kind == "bubble" else ops._pcsaft_mix_dew
        return _run(entry, [params, comp, kij, eab, owner, states[:, 0], states[:, 2:]], n,
                    [(n,), (n, nc), (n,), (n,)])
    inputs = [params, comp, kij, eab, owner, states[:, 0], states[:, 1], states[:, 2:]]
    if kind == "density":
        return _run(ops._pcsaft_mix, inputs, n, [(n,)], name="pcsaft_mix_density")
    pure = kind == "lnphi_pure"
    return _run(ops._pcsaft_mix, inputs, n, [(n,), (n, nc), (n, nc) if pure else None], name="pcsaft_mix_lnphi", last=pure)


def _square(matrix: Any, k: int, nc: int, fill: float, what: str) -> np.ndarray:
    """a [k, k] matrix placed in the corner of an [nc, nc] one"""
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (k, k):
        raise ValueError(f"{what} must be a {k} x {k} matrix, got shape {m.shape}")
    out = np.full((nc, nc), fill, dtype=np.float64)
    out[:k, :k] = m
    return out


def _pool(mixtures: Sequence[Sequence[Sequence[float]]], kij: Optional[Sequence[Any]], eab: Optional[Sequence[Any]]):
    """pools the component rows of all mixtures: (params [B, 9], comp [M, nc], kij, eab [M, nc, nc] or None)"""
    sizes = [len(rows) for rows in mixtures]
    if not sizes or min(sizes) < 1 or max(sizes) > NC_MAX:
        raise ValueError(f"a mixture has 1 to {NC_MAX} components, got {sizes}")
    nc, M = max(sizes), len(mixtures)
    params = np.concatenate([_rows(rows) for rows in mixtures])
    comp = np.full((M, nc), -1, dtype=np.int64)
    start = 0
    for i, k in enumerate(sizes):
        comp[i, :k] = np.arange(start, start + k)
        start += k

    def stack(mats, fill, what):
        if mats is None or all(m is None for m in mats):
            return None
        if len(mats) != M:
            raise ValueError(f"{len(mats)} {what} matrices for {M} mixtures")
        return np.stack([np.full((nc, nc), fill) if m is None else _square(m, k, nc, fill, what)
                         for m, k in zip(mats, sizes)])

    return params, comp, stack(kij, 0.0, "kij"), stack(eab, np.nan, "epsilon_ab")


def _states(table: Any, k: int, nc: int) -> np.ndarray:
    """[rows, 2 + k] state table [T, P, x1..xk] widened to nc composition columns"""
    t = np.asarray(table, dtype=np.float64)
    t = t.reshape(t.shape[0], -1)
    if t.shape[1] != 2 + k:
        raise ValueError(f"a state row of a {k}-component mixture is [T, P, x1..x{k}], got {t.shape[1]} values")
    out = np.zeros((t.shape[0], 2 + nc), dtype=np.float64)
    out[:, :2 + k] = t
    return out


def _mix_batch(kind: str, mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]], pick
               ) -> List[Tuple[int, np.ndarray]]:
    """The mixture batch forms: (i, rows of ``pick(values of _run_mix)``) of every non-empty table i, in one launch"""
    tables = _nonempty("mixtures", len(mixtures), states_batch)
    if not tables:
        return []
    params, comp, d_kij, _ = _pool(mixtures, kij, None)
    index = [i for i, _ in tables]
    states = [_states(s, len(mixtures[i]), comp.shape[1]) for i, s in tables]
    parts = _run_tables(index, states, lambda owner, st: pick(_run_mix(kind, params, comp, d_kij, None, owner, st)[0]))
    return list(zip(index, parts))


def mix_rho_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None
                  ) -> List[np.ndarray]:
    """Liquid densities (mol/m³) of every state of every non-empty table in one launch: ``mixtures[i]`` is the list of
    component rows of system i, ``states_batch[i]`` its array of rows ``[T (K), P (Pa), x1..x_nc]``, ``kij[i]`` its
    k_ij matrix or None.  One fp64 array per non-empty table, 0.0 where a point failed (the double loop of the
    reference's demo/utils_binary.py ``binary_test`` as one call)."""
    return [v.copy() for _, v in _mix_batch("density", mixtures, states_batch, kij, lambda values: values[0])]


def _mix_point(what: str, kind: str, parameters: Sequence[Sequence[float]], state: Sequence[float],
               kij_matrix: Optional[Any], epsilon_ab: Optional[Any], start: Optional[float] = None
               ) -> Tuple[List[Optional[np.ndarray]], np.ndarray]:
    """(values of ``_run_mix``, the state row [1, 2 + nc]) of one point; RuntimeError on a status != 0.  ``start``: the
    start temperature of the kinds that take one."""
    params, comp, kij, eab = _pool([parameters], [kij_matrix], [epsilon_ab])
    states = _states([list(state)], len(parameters), comp.shape[1])
    first = None if start is None else np.asarray([start], dtype=np.float64)
    values, status = _run_mix(kind, params, comp, kij, eab, np.zeros(1, dtype=np.int64), states, first)
    _require_ok(status, f"mixture {what}", state)
    return values, states


def mix_den(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
            epsilon_ab: Optional[Any] = None) -> float:
    """Mixture liquid density (mol/m³) at ``state = [T (K), P (Pa), x1, x2, ...]`` of the components ``parameters``
    (reference ``mix_den_feos``); raises ``RuntimeError`` where no liquid root is found."""
    (rho,), _ = _mix_point("density", "density", parameters, state, kij_matrix, epsilon_ab)
    return float(rho[0])


def _phi_point(what: str, parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any],
               epsilon_ab: Optional[Any], pure: bool) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray]:
    """(lnphi [k], lnphi_pure [k] or None, x [k] normalised by its sum) of one point; RuntimeError on a status != 0"""
    k = len(parameters)
    (_, lnphi, lnphi_pure), states = _mix_point(what, "lnphi_pure" if pure else "lnphi", parameters, state, kij_matrix,
                                                 epsilon_ab)
    x = states[0, 2:2 + k]
    return lnphi[0, :k], None if lnphi_pure is None else lnphi_pure[0, :k], x / x.sum()


def mix_ln_fugacity_coefficient(parameters: Sequence[Sequence[float]], state: Sequence[float],
                                kij_matrix: Optional[Any] = None, epsilon_ab: Optional[Any] = None) -> np.ndarray:
    """ln phi_i of every component at the liquid root of ``state = [T (K), P (Pa), x1, x2, ...]`` (reference
    ``mix_ln_fugacity_coefficient``), the infinite-dilution value where x_i = 0; raises ``RuntimeError`` where no liquid
    root is found."""
    return _phi_point("fugacity coefficient", parameters, state, kij_matrix, epsilon_ab, False)[0]


def mix_ln_fugacity_coefficient_pure(parameters: Sequence[Sequence[float]], state: Sequence[float],
                                     kij_matrix: Optional[Any] = None, epsilon_ab: Optional[Any] = None) -> np.ndarray:
    """ln phi of every component alone at its own liquid root at the T and P of ``state`` (reference
    ``mix_ln_fugacity_coefficient_pure``); NaN for a component without a liquid root there."""
    return _phi_point("fugacity coefficient", parameters, state, kij_matrix, epsilon_ab, True)[1]


def _activity(parameters, state, kij_matrix, epsilon_ab) -> Tuple[np.ndarray, np.ndarray]:
    lnphi, lnphi_pure, x = _phi_point("activity coefficient", parameters, state, kij_matrix, epsilon_ab, True)
    if np.any(np.isnan(lnphi_pure)):
        raise RuntimeError(f"PC-SAFT mixture activity coefficient failed at state {list(state)}: component(s) "
                           f"{np.nonzero(np.isnan(lnphi_pure))[0].tolist()} have no liquid root of their own")
    return lnphi - lnphi_pure, x


def mix_ln_activity_coefficient(parameters: Sequence[Sequence[float]], state: Sequence[float],
                                kij_matrix: Optional[Any] = None, epsilon_ab: Optional[Any] = None) -> np.ndarray:
    """ln gamma_i = ln phi_i - ln phi_i^pure (symmetric convention, reference ``mix_ln_activity_coefficient``); raises
    ``RuntimeError`` where the mixture or one of its components alone has no liquid root."""
    return _activity(parameters, state, kij_matrix, epsilon_ab)[0]


def mix_e_gibbs_energy(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
                       epsilon_ab: Optional[Any] = None) -> float:
    """Molar excess Gibbs energy g^E/RT = sum_i x_i ln gamma_i (reference ``mix_e_gibbs_energy``)."""
    ln_gamma, x = _activity(parameters, state, kij_matrix, epsilon_ab)
    return float(np.sum(ln_gamma * x))


def mix_r_gibbs_energy(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
                       epsilon_ab: Optional[Any] = None) -> float:
    """Molar residual Gibbs energy g^res/RT = sum_i x_i ln phi_i (reference ``mix_r_gibbs_energy``)."""
    lnphi, _, x = _phi_point("fugacity coefficient", parameters, state, kij_matrix, epsilon_ab, False)
    return float(np.sum(lnphi * x))


def mix_gibbs_energy(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
                     epsilon_ab: Optional[Any] = None) -> float:
    """Molar Gibbs energy of mixing g/RT = g^E/RT + sum_i x_i ln x_i (reference ``mix_gibbs_energy``), with 0 ln 0 = 0."""
    ln_gamma, x = _activity(parameters, state, kij_matrix, epsilon_ab)
    present = x > 0
    return float(np.sum(ln_gamma * x) + np.sum(x[present] * np.log(x[present])))


def mix_ln_phi_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None,
                     activity: bool = False) -> List[np.ndarray]:
    """ln phi_i of every state of every non-empty table in one launch, arguments as ``mix_rho_batch``: one fp64 array
    [rows, nc_i] per non-empty table, a row of NaN where a point failed.  With ``activity`` the arrays hold ln gamma_i
    = ln phi_i - ln phi_i^pure instead (NaN where a component has no liquid root of its own)."""
    def pick(values):
        return values[1] - values[2] if activity else values[1]

    parts = _mix_batch("lnphi_pure" if activity else "lnphi", mixtures, states_batch, kij, pick)
    return [v[:, :len(mixtures[i])].copy() for i, v in parts]


def _failed_nan(values: np.ndarray, P: np.ndarray) -> np.ndarray:
    """rows of NaN where a bubble or dew point failed (P = 0.0)"""
    return np.where((P > 0.0)[:, None], values, np.nan)


def mix_bubble(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
               epsilon_ab: Optional[Any] = None) -> Tuple[float, np.ndarray]:
    """Bubble point of the liquid ``state = [T (K), P, x1, x2, ...]`` (P is ignored) of the components ``parameters``:
    (P (Pa), y [k]), the bubble half of the reference's ``mix_vp_feos``; raises ``RuntimeError`` where there is no
    bubble point at this T or the solve does not converge."""
    (P, y, _, _), _ = _mix_point("bubble point", "bubble", parameters, state, kij_matrix, epsilon_ab)
    return float(P[0]), y[0, :len(parameters)].copy()


def mix_bubble_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None
                     ) -> List[np.ndarray]:
    """Bubble points of every state of every non-empty table in one launch, arguments as ``mix_rho_batch`` (the P column
    is ignored): one fp64 array [rows, 1 + nc_i] of rows ``[P (Pa), y1..y_nc]`` per non-empty table, a row of NaN where a
    point failed."""
    def pick(values):
        return _failed_nan(np.concatenate([values[0][:, None], values[1]], axis=1), values[0])

    parts = _mix_batch("bubble", mixtures, states_batch, kij, pick)
    return [v[:, :1 + len(mixtures[i])].copy() for i, v in parts]


def mix_dew(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
            epsilon_ab: Optional[Any] = None) -> Tuple[float, np.ndarray]:
    """Dew point of the vapour ``state = [T (K), P, y1, y2, ...]`` (P is ignored) of the components ``parameters``:
    (P (Pa), x [k]), the dew half of the reference's ``mix_vp_feos``; raises ``RuntimeError`` where no dew point is found
    at this T or the solve does not converge."""
    (P, x, _, _), _ = _mix_point("dew point", "dew", parameters, state, kij_matrix, epsilon_ab)
    return float(P[0]), x[0, :len(parameters)].copy()


def mix_dew_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None
                  ) -> List[np.ndarray]:
    """Dew points of every state of every non-empty table in one launch, arguments as ``mix_bubble_batch`` (the
    composition columns hold the vapour): one fp64 array [rows, 1 + nc_i] of rows ``[P (Pa), x1..x_nc]`` per non-empty
    table, a row of NaN where a point failed."""
    def pick(values):
        return _failed_nan(np.concatenate([values[0][:, None], values[1]], axis=1), values[0])

    parts = _mix_batch("dew", mixtures, states_batch, kij, pick)
    return [v[:, :1 + len(mixtures[i])].copy() for i, v in parts]


def mix_vp(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
           epsilon_ab: Optional[Any] = None) -> Tuple[float, float]:
    """(bubble pressure, dew pressure) in Pa of the composition in ``state = [T (K), P, z1, z2, ...]`` (P is ignored),
    the reference's ``mix_vp_feos``: the composition is the liquid of the bubble point and the vapour of the dew point.
    The numbers are those of ``mix_bubble`` and ``mix_dew``; raises ``RuntimeError`` where either fails."""
    return (mix_bubble(parameters, state, kij_matrix, epsilon_ab)[0],
            mix_dew(parameters, state, kij_matrix, epsilon_ab)[0])


def mix_vle_pxy(parameters: Sequence[Sequence[float]], temperature: float, kij_matrix: Optional[Any] = None,
                epsilon_ab: Optional[Any] = None, points: int = 51) -> dict:
    """P-x-y diagram of a binary at ``temperature`` (reference ``mix_vle_pxy_diagram_feos``): the bubble points at
    x_first = linspace(0, 1, points) in one launch, as a dict of equally long lists under the keys ``temperature``,
    ``pressure`` (Pa), ``density liquid``, ``density vapor`` (mol/m³), ``x0``, ``x1``, ``y0``, ``y1`` (x0, y0: the first
    component).  Points without a bubble point (beyond the critical composition) are dropped; ``ValueError`` if none is
    left, and for anything but two components.  The dew curve is y(x) along these points."""
    if len(parameters) != 2:
        raise ValueError(f"a P-x-y diagram needs a binary mixture, got {len(parameters)} components")
    if int(points) < 2:
        raise ValueError(f"a P-x-y diagram needs at least 2 points, got {points}")
    params, comp, kij, eab = _pool([parameters], [kij_matrix], [epsilon_ab])
    x0 = np.linspace(0.0, 1.0, int(points))
    states = _states(np.stack([np.full_like(x0, float(temperature)), np.zeros_like(x0), x0, 1.0 - x0], axis=1), 2, 2)
    (P, y, rho_l, rho_v), status = _run_mix("bubble", params, comp, kij, eab, np.zeros(len(x0), dtype=np.int64), states)
    keep = status == STATUS_OK
    if not keep.any():
        raise ValueError("No VLE found at the given conditions.")
    return {"temperature": states[keep, 0].tolist(), "pressure": P[keep].tolist(),
            "density liquid": rho_l[keep].tolist(), "density vapor": rho_v[keep].tolist(),
            "x0": x0[keep].tolist(), "x1": (1.0 - x0)[keep].tolist(),
            "y0": y[keep, 0].tolist(), "y1": y[keep, 1].tolist()}


def mix_bubble_t(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
                 epsilon_ab: Optional[Any] = None, t_init: Optional[float] = None) -> Tuple[float, np.ndarray]:
    """Bubble temperature of the liquid ``state = [T, P (Pa), x1, x2, ...]`` (T is ignored) of the components
    ``parameters``: (T (K), y [k]), feos ``PhaseEquilibrium.bubble_point`` at given pressure.  ``t_init``: the temperature
    the solve starts from (feos ``tp_init``), None for the kernel's own start.  Raises ``RuntimeError`` where no bubble
    temperature is found at this P or the solve does not converge."""
    (T, y, _, _), _ = _mix_point("bubble temperature", "bubble_t", parameters, state, kij_matrix, epsilon_ab, t_init)
    return float(T[0]), y[0, :len(parameters)].copy()


def mix_dew_t(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
              epsilon_ab: Optional[Any] = None, t_init: Optional[float] = None) -> Tuple[float, np.ndarray]:
    """Dew temperature of the vapour ``state = [T, P (Pa), y1, y2, ...]`` (T is ignored): (T (K), x [k]), feos
    ``PhaseEquilibrium.dew_point`` at given pressure; arguments and errors as ``mix_bubble_t``.  A vapour can have more
    than one dew temperature: the one reported is the one the start leads to."""
    (T, x, _, _), _ = _mix_point("dew temperature", "dew_t", parameters, state, kij_matrix, epsilon_ab, t_init)
    return float(T[0]), x[0, :len(parameters)].copy()


def _t_batch(kind: str, mixtures, states_batch, kij) -> List[np.ndarray]:
    def pick(values):
        return _failed_nan(np.concatenate([values[0][:, None], values[1]], axis=1), values[0])

    parts = _mix_batch(kind, mixtures, states_batch, kij, pick)
    return [v[:, :1 + len(mixtures[i])].copy() for i, v in parts]


def mix_bubble_t_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None
                       ) -> List[np.ndarray]:
    """Bubble temperatures of every state of every non-empty table in one launch, arguments as ``mix_bubble_batch`` (the
    T column is ignored, the P column read): one fp64 array [rows, 1 + nc_i] of rows ``[T (K), y1..y_nc]`` per non-empty
    table, a row of NaN where a point failed."""
    return _t_batch("bubble_t", mixtures, states_batch, kij)


def mix_dew_t_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None
                    ) -> List[np.ndarray]:
    """Dew temperatures of every state of every non-empty table in one launch, arguments as ``mix_bubble_t_batch`` (the
    composition columns hold the vapour): rows ``[T (K), x1..x_nc]``, a row of NaN where a point failed."""
    return _t_batch("dew_t", mixtures, states_batch, kij)


def mix_vle_txy(parameters: Sequence[Sequence[float]], pressure: float, kij_matrix: Optional[Any] = None,
                epsilon_ab: Optional[Any] = None, points: int = 51) -> dict:
    """T-x-y diagram of a binary at ``pressure`` (Pa) (reference ``mix_vle_diagram_feos``): the bubble temperatures at
    x_first = linspace(0, 1, points) in one launch, as a dict of the keys of ``mix_vle_pxy``.  Points without a bubble
    temperature (a pressure above the critical one at that composition) are dropped; ``ValueError`` if none is left, and
    for anything but two components.  The dew curve is y(x) along these points."""
    if len(parameters) != 2:
        raise ValueError(f"a T-x-y diagram needs a binary mixture, got {len(parameters)} components")
    if int(points) < 2:
        raise ValueError(f"a T-x-y diagram needs at least 2 points, got {points}")
    params, comp, kij, eab = _pool([parameters], [kij_matrix], [epsilon_ab])
    x0 = np.linspace(0.0, 1.0, int(points))
    states = _states(np.stack([np.zeros_like(x0), np.full_like(x0, float(pressure)), x0, 1.0 - x0], axis=1), 2, 2)
    (T, y, rho_l, rho_v), status = _run_mix("bubble_t", params, comp, kij, eab, np.zeros(len(x0), dtype=np.int64), states)
    keep = status == STATUS_OK
    if not keep.any():
        raise ValueError("No VLE found at the given conditions.")
    return {"temperature": T[keep].tolist(), "pressure": states[keep, 1].tolist(),
            "density liquid": rho_l[keep].tolist(), "density vapor": rho_v[keep].tolist(),
            "x0": x0[keep].tolist(), "x1": (1.0 - x0)[keep].tolist(),
            "y0": y[keep, 0].tolist(), "y1": y[keep, 1].tolist()}


def mix_tp_flash(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
                 epsilon_ab: Optional[Any] = None) -> dict:
    """Two-phase flash of the feed ``state = [T (K), P (Pa), z1, z2, ...]`` of the components ``parameters`` (reference
    ``mix_tp_flash_feos``): a dict with ``beta`` (the vapour mole fraction), ``x``, ``y`` ([k] arrays, liquid and vapour)
    and ``density liquid``, ``density vapor`` (mol/m³); raises ``RuntimeError`` where the feed does not split into a
    vapour and a liquid at (T, P) or the solve does not converge."""
    (beta, x, y, rho_l, rho_v), _ = _mix_point("flash", "flash", parameters, state, kij_matrix, epsilon_ab)
    k = len(parameters)
    return {"beta": float(beta[0]), "x": x[0, :k].copy(), "y": y[0, :k].copy(), "density liquid": float(rho_l[0]),
            "density vapor": float(rho_v[0])}


def mix_tp_flash_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None
                       ) -> List[np.ndarray]:
    """Flashes of every state of every non-empty table in one launch, arguments as ``mix_rho_batch`` (the composition
    columns hold the feed): one fp64 array [rows, 1 + 2 nc_i] of rows ``[beta, x1..x_nc, y1..y_nc]`` per non-empty table, a
    row of NaN where a point has no vapour-liquid split or failed."""
    def pick(values):
        row = np.concatenate([values[0][:, None], values[1], values[2]], axis=1)
        return np.where(np.isnan(values[1][:, :1]), np.nan, row)  # the first slot is always used: NaN there = failed

    parts = _mix_batch("flash", mixtures, states_batch, kij, pick)
    out = []
    for i, v in parts:
        k, nc = len(mixtures[i]), (v.shape[1] - 1) // 2
        out.append(np.concatenate([v[:, :1 + k], v[:, 1 + nc:1 + nc + k]], axis=1))
    return out


def mix_flash_x1(parameters: Sequence[Sequence[float]], states: Any, feed_x1s: Any, kij_matrix: Optional[Any] = None,
                 epsilon_ab: Optional[Any] = None) -> np.ndarray:
    """x_1 of the denser phase of a binary at every row ``[T (K), P (Pa)]`` of ``states`` [n, 2]: all n x F flashes of the
    trial feeds z_1 = ``feed_x1s`` [F] run in one launch, and each state takes the first feed, in order, that splits
    (status 0); NaN where none does -> [n] fp64 (the loop of the reference's pcsaft/kij.py ``_pred_x1_worker``, which tries
    the feeds one by one).  The denser phase is the liquid: rho_l > rho_v wherever the status is 0.  ``ValueError`` for
    anything but two components."""
    if len(parameters) != 2:
        raise ValueError(f"mix_flash_x1 needs a binary mixture, got {len(parameters)} components")
    st = np.asarray(states, dtype=np.float64)
    feeds = np.asarray(feed_x1s, dtype=np.float64)
    if st.ndim != 2 or st.shape[1] != 2:
        raise ValueError(f"states must be [n, 2] rows of [T, P], got shape {st.shape}")
    if feeds.ndim != 1 or feeds.size == 0:
        raise ValueError(f"feed_x1s must be a non-empty 1-d array, got shape {feeds.shape}")
    params, comp, kij, eab = _pool([parameters], [kij_matrix], [epsilon_ab])
    n, F = st.shape[0], feeds.size
    if n == 0:
        return np.zeros(0, dtype=np.float64)
    z1 = np.tile(feeds, n)
    points = np.concatenate([np.repeat(st, F, axis=0), z1[:, None], 1.0 - z1[:, None]], axis=1)
    (_, x, _, _, _), status = _run_mix("flash", params, comp, kij, eab, np.zeros(n * F, dtype=np.int64), points)
    ok = (status == STATUS_OK).reshape(n, F)
    first = np.argmax(ok, axis=1)
    return np.where(ok.any(axis=1), x[:, 0].reshape(n, F)[np.arange(n), first], np.nan)


def mix_is_stable(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
                  epsilon_ab: Optional[Any] = None, density_initialization: Optional[str] = None) -> bool:
    """Is the feed ``state = [T (K), P (Pa), z1, z2, ...]`` of the components ``parameters`` one stable phase (reference
    ``is_stable_feos``)?  False where one of the nc + 2 trial phases has a negative tangent-plane distance.  The state of
    the feed is the one of its liquid and vapour roots with the lower Gibbs energy, feos's
    ``density_initialization=None``, which is what the reference passes: any other value raises ``ValueError``.  Raises
    ``RuntimeError`` where the test is inconclusive (a trial without a root or an end, and none that is negative)."""
    if density_initialization is not None:
        raise ValueError(f"mix_is_stable takes the feed's state of lower Gibbs energy (density_initialization=None), got "
                         f"{density_initialization!r}")
    (tpd, _), _ = _mix_point("stability", "stability", parameters, state, kij_matrix, epsilon_ab)
    return bool(tpd[0] >= 0.0)


def mix_stability_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None
                        ) -> List[np.ndarray]:
    """Stability tests of every state of every non-empty table in one launch, arguments as ``mix_rho_batch`` (the
    composition columns hold the feed): one fp64 array [rows, 1 + nc_i] of rows ``[tpd, w1..w_nc]`` per non-empty table.
    tpd < 0: unstable, w the trial composition with the most negative tangent-plane distance; tpd >= 0: stable, the
    smallest stationary distance and its w (0.0 and the feed where every trial fell onto the feed); a row of NaN where
    a point is inconclusive."""
    parts = _mix_batch("stability", mixtures, states_batch, kij,
                       lambda values: np.concatenate([values[0][:, None], values[1]], axis=1))
    return [v[:, :1 + len(mixtures[i])].copy() for i, v in parts]


def _lle_dict(k: int, states: np.ndarray, values: List[np.ndarray], keep: np.ndarray) -> dict:
    """the reference's LLE dict of the points ``keep``: the keys of ``mix_vle_txy`` for k components, and ``beta``"""
    beta, x, y, rho_x, rho_y = values
    out = {"temperature": states[keep, 0].tolist(), "pressure": states[keep, 1].tolist(),
           "density liquid": rho_x[keep].tolist(), "density vapor": rho_y[keep].tolist()}
    out.update({f"x{j}": x[keep, j].tolist() for j in range(k)})
    out.update({f"y{j}": y[keep, j].tolist() for j in range(k)})
    out["beta"] = beta[keep].tolist()
    return out


def mix_lle(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
            epsilon_ab: Optional[Any] = None) -> dict:
    """Liquid-liquid split of the feed ``state = [T (K), P (Pa), z1, z2, ...]`` of the components ``parameters``
    (reference ``mix_lle_feos``): the stability test, then the split started from its w.  A dict of one-element lists
    under the keys of ``mix_vle_txy`` for k components (``temperature``, ``pressure``, ``density liquid``, ``density
    vapor`` in mol/m³, ``x0..x{k-1}``, ``y0..y{k-1}``) and ``beta``, the mole fraction of phase 2.  As in the reference,
    "vapor" and y name liquid phase 2; "liquid" and x are the phase of higher molar density.  Raises ``ValueError`` where
    no split is found (a stable feed, or a solve that does not end)."""
    return mix_lle_diagram(parameters, state, kij_matrix, epsilon_ab, points=1)


def mix_lle_diagram(parameters: Sequence[Sequence[float]], state: Sequence[float], kij_matrix: Optional[Any] = None,
                    epsilon_ab: Optional[Any] = None, points: int = 200) -> dict:
    """Liquid-liquid diagram of the feed ``state = [T (K), P (Pa), z1, z2, ...]`` at P and T = linspace(T, T + 50,
    points) (reference ``mix_lle_diagram_feos``): one stability launch and one split launch for all temperatures, as a
    dict of equally long lists under the keys of ``mix_lle``.  Points without a split are dropped; ``ValueError`` if none
    is left.  ``points`` = 1 is the feed's own temperature alone."""
    if int(points) < 1:
        raise ValueError(f"a liquid-liquid diagram needs at least 1 point, got {points}")
    params, comp, kij, eab = _pool([parameters], [kij_matrix], [epsilon_ab])
    k = len(parameters)
    one = _states([list(state)], k, comp.shape[1])
    states = np.repeat(one, int(points), axis=0)
    if int(points) > 1:
        states[:, 0] = np.linspace(one[0, 0], one[0, 0] + 50.0, int(points))
    values, status = _run_mix("lle", params, comp, kij, eab, np.zeros(len(states), dtype=np.int64), states)
    keep = status == STATUS_OK
    if not keep.any():
        raise ValueError("No LLE found at the given conditions.")
    return _lle_dict(k, states, values, keep)


def mix_lle_batch(mixtures: List[List[List[Any]]], states_batch: List[Any], kij: Optional[List[Any]] = None
                  ) -> List[np.ndarray]:
    """Liquid-liquid splits of every state of every non-empty table in two launches (the stability test, then the
    split), arguments as ``mix_tp_flash_batch``: one fp64 array [rows, 1 + 2 nc_i] of rows ``[beta, x1..x_nc, y1..y_nc]``
    per non-empty table, x the phase of higher molar density; a row of NaN where a point has no split or failed."""
    def pick(values):
        row = np.concatenate([values[0][:, None], values[1], values[2]], axis=1)
        return np.where(np.isnan(values[1][:, :1]), np.nan, row)  # the first slot is always used: NaN there = failed

    parts = _mix_batch("lle", mixtures, states_batch, kij, pick)
    out = []
    for i, v in parts:
        k, nc = len(mixtures[i]), (v.shape[1] - 1) // 2
        out.append(np.concatenate([v[:, :1 + k], v[:, 1 + nc:1 + nc + k]], axis=1))
    return out


# ---- the k_ij fit of binaries (csrc/gnx_pcsaft_kij.hip; reference pcsaft/kij.py) --------------------------
KIJ_COLUMNS = ("inchi1", "inchi2", "T_K", "P_kPa", "mole_fraction_c1p2")
KIJ_KEYS = ("inchi1", "inchi2", "k_12", "loss", "loss_nonan", "mape", "n_nan")
CO2_INCHI = "InChI=1S/CO2/c2-1-3"
_CO2_TC, _CO2_PC_KPA = 304.2, 7377.3  # the reference's CO2 check: below Tc the vapour pressure, from Tc on this


def _kij_matrices(k12: np.ndarray) -> np.ndarray:
    """[C] values of k_12 -> [C, 2, 2] symmetric matrices with a zero diagonal"""
    out = np.zeros((k12.shape[0], 2, 2), dtype=np.float64)
    out[:, 0, 1] = out[:, 1, 0] = k12
    return out


def _run_kij_x1(inputs: Sequence[Optional[np.ndarray]], n: int
                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """One upload, one ``ops._pcsaft_kij_x1`` launch and one download of (x1, feed, residual, status) [n]"""
    def entry(*args, out):  # the buffer of _run_packed holds the fp64 outputs first; the entry has the feed between them
        return ops._pcsaft_kij_x1(*args, out=(out[0], out[2], out[1], out[3]))

    (x1, residual), (feed, status) = _run_packed(entry, inputs, n, [(n,), (n,)], ints=2)
    return x1, feed, residual, status


def mix_kij_x1(parameters: Sequence[Sequence[float]], states: Any, x1_exp: Any, feed_x1s: Any, k12s: Any,
               epsilon_ab: Optional[Any] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``mix_flash_x1`` of one binary under every candidate k_12 of ``k12s`` [C] in one launch, with the residual of the
    fit: ``states`` [n, 2] rows ``[T (K), P (Pa)]``, ``x1_exp`` [n] the measured liquid x_1, ``feed_x1s`` [F] the trial
    feeds -> (x1 [C, n] of the first feed, in order, that splits; feed [C, n] int32 its index; residual [C, n] =
    log((x1 + 1e-6) / (x1_exp + 1e-6)); status [C, n] int32).  Where no feed splits: NaN, -1, the reference's penalty 10.0
    and a status != 0.  One wave per (candidate, state) and one lane per feed (csrc/gnx_pcsaft_kij.hip); x1 is bit for bit
    what ``mix_flash_x1`` returns under that k_12.  Like ``mix_flash_x1`` and unlike the reference's ``_pred_x1_worker``,
    no stability test runs before a flash: a stable feed has no split with beta in [0, 1] and the flash reports it as single
    phase.  Liquid-liquid splits are not looked for.  ``ValueError`` for anything but two components."""
    if len(parameters) != 2:
        raise ValueError(f"mix_kij_x1 needs a binary mixture, got {len(parameters)} components")
    st = np.asarray(states, dtype=np.float64)
    xe = np.asarray(x1_exp, dtype=np.float64)
    feeds = np.ascontiguousarray(feed_x1s, dtype=np.float64)
    ks = np.asarray(k12s, dtype=np.float64)
    if st.ndim != 2 or st.shape[1] != 2:
        raise ValueError(f"states must be [n, 2] rows of [T, P], got shape {st.shape}")
    if xe.shape != (st.shape[0],):
        raise ValueError(f"x1_exp must be [{st.shape[0]}], one value per state, got shape {xe.shape}")
    if feeds.ndim != 1 or feeds.size == 0:
        raise ValueError(f"feed_x1s must be a non-empty 1-d array, got shape {feeds.shape}")
    if ks.ndim != 1:
        raise ValueError(f"k12s must be a 1-d array, got shape {ks.shape}")
    params = _rows(parameters)
    eab = None if epsilon_ab is None else np.repeat(_square(epsilon_ab, 2, 2, np.nan, "epsilon_ab")[None], ks.size, axis=0)
    n, C = st.shape[0], ks.size
    if n * C == 0:
        return (np.zeros((C, n)), np.zeros((C, n), dtype=np.int32), np.zeros((C, n)), np.zeros((C, n), dtype=np.int32))
    comp = np.tile(np.arange(2, dtype=np.int64), (C, 1))
    owner = np.repeat(np.arange(C, dtype=np.int64), n)
    out = _run_kij_x1([params, comp, _kij_matrices(ks), eab, owner, np.tile(st[:, 0], C), np.tile(st[:, 1], C),
                       np.tile(xe, C), feeds], n * C)
    return tuple(v.reshape(C, n) for v in out)


def _fit_kij_core(evaluate, npts: Any, k0: float = 0.2, xtol: float = 1e-8, ftol: float = 1e-8, max_iter: int = 50
                  ) -> dict:
    """Levenberg-Marquardt in one parameter for S independent problems in lockstep.  ``evaluate(index [A] int64, k [A])``
    -> sums [A, 8] fp64 of ``ops.pcsaft_kij_sums`` for the systems ``index`` at k (and at k plus the difference step,
    which is the evaluator's business): slot 0 sum r^2, 1 the penalised rows, 2 sum |r| and 3 sum |pred - x1| / x1 of the
    others, 5 sum J r, 6 sum J^2.  ``npts`` [S]: the rows of each system.

    lambda starts at 1e-3; the trial step is -sum J r / (sum J^2 (1 + lambda)).  A trial whose cost 0.5 sum r^2 does not
    rise is accepted with lambda / 10, and its Jacobian came with it; a rejected one sets lambda * 10 and the step is
    taken again from the kept Jacobian.  A system ends, and is in no later call of ``evaluate``, with the reason "cost 0",
    "flat" (sum J^2 == 0: nothing to differentiate), "xtol" (|step| < xtol (xtol + |k|)), "ftol" (an accepted decrease <=
    ftol cost), "lambda" (lambda > 1e12) or "max_iter" (evaluations after the first).  Everything is elementwise over the
    systems: one fitted with others gets the bits it gets alone.  -> dict of [S] arrays ``k_12``, ``loss`` (mean r^2),
    ``loss_nonan`` (mean |r| of the unpenalised rows, 1.0 without any), ``mape`` (mean |pred - x1| / x1 likewise),
    ``n_nan``, ``iterations``, ``reason``, all of the last accepted evaluation."""
    npts = np.asarray(npts, dtype=np.int64)
    S = npts.shape[0]
    k = np.full(S, float(k0), dtype=np.float64)
    lam = np.full(S, 1e-3, dtype=np.float64)
    iters = np.zeros(S, dtype=np.int64)
    reason = np.full(S, "", dtype=object)
    sums = np.zeros((S, 8), dtype=np.float64)
    if S:
        sums[:] = np.asarray(evaluate(np.arange(S, dtype=np.int64), k.copy()), dtype=np.float64).reshape(S, 8)
    reason[sums[:, 6] == 0.0] = "flat"
    reason[sums[:, 0] == 0.0] = "cost 0"
    while True:
        idx = np.flatnonzero(reason == "")
        late = idx[iters[idx] >= max_iter]
        reason[late] = "max_iter"
        idx = idx[iters[idx] < max_iter]
        if idx.size == 0:
            break
        cost = 0.5 * sums[idx, 0]
        step = -sums[idx, 5] / (sums[idx, 6] * (1.0 + lam[idx]))
        trial = np.asarray(evaluate(idx, k[idx] + step), dtype=np.float64).reshape(idx.size, 8)
        iters[idx] += 1
        new = 0.5 * trial[:, 0]
        ok = new <= cost  # False for a NaN cost
        small = np.abs(step) < xtol * (xtol + np.abs(k[idx]))
        acc, rej = idx[ok], idx[~ok]
        k[acc] += step[ok]
        sums[acc] = trial[ok]
        lam[acc] /= 10.0
        lam[rej] *= 10.0
        why = np.full(idx.size, "", dtype=object)
        why[~ok & (lam[idx] > 1e12)] = "lambda"
        why[ok & (cost - new <= ftol * cost)] = "ftol"
        why[small] = "xtol"  # accepted or not: a larger lambda only shortens the step
        why[ok & (trial[:, 6] == 0.0)] = "flat"
        why[ok & (new == 0.0)] = "cost 0"
        reason[idx] = why
    good = npts - sums[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"k_12": k, "loss": sums[:, 0] / npts,
                "loss_nonan": np.where(good > 0, sums[:, 2] / good, 1.0), "mape": np.where(good > 0, sums[:, 3] / good, 1.0),
                "n_nan": np.where(np.isfinite(sums[:, 1]), sums[:, 1], npts).astype(np.int64),  # NaN sums: no row counts
                "iterations": iters, "reason": reason}


def _kij_systems(systems: Sequence[Any]) -> Tuple[np.ndarray, List[np.ndarray], List[np.ndarray], List[np.ndarray]]:
    """(params [2 S, 9], T, P, x1: one [n_s] fp64 array per system) of ``fit_kij``'s systems, checked"""
    rows, Ts, Ps, xs = [], [], [], []
    for s, (parameters, T, P, x1) in enumerate(systems):
        if len(parameters) != 2:
            raise ValueError(f"system {s}: the k_ij fit needs a binary mixture, got {len(parameters)} components")
        rows.append(_rows(parameters))
        T, P, x1 = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (T, P, x1))
        if not T.size or T.shape != P.shape or T.shape != x1.shape:
            raise ValueError(f"system {s}: T, P and x1 must be equally long and not empty, got {T.size}, {P.size}, {x1.size}")
        Ts.append(T)
        Ps.append(P)
        xs.append(x1)
    return (np.concatenate(rows) if rows else np.zeros((0, 9))), Ts, Ps, xs


def _kij_evaluator(systems: Sequence[Any], feeds: np.ndarray, diff_step: float):
    """(evaluate, npts) for ``_fit_kij_core`` on the GPU: parameters and feeds are uploaded once; ``evaluate(index, k)`` is
    one upload of the rows [system][k, k + diff_step][point] of the systems ``index``, one ``ops.pcsaft_kij_x1`` and one
    ``ops.pcsaft_kij_sums`` launch and one download of [len(index), 8]."""
    params, Ts, Ps, xs = _kij_systems(systems)
    npts = np.array([t.size for t in Ts], dtype=np.int64)
    if not len(Ts):
        return None, npts
    dev = _device()
    d_params, d_feeds = _upload(dev, [params, feeds])
    h = float(diff_step)

    def evaluate(index: np.ndarray, k: np.ndarray) -> np.ndarray:
        A = index.size
        comp = np.repeat(2 * index, 2)[:, None] + np.arange(2, dtype=np.int64)  # candidates share their component rows
        kij = _kij_matrices(np.stack([k, k + h], axis=1).reshape(-1))
        n_a = npts[index]
        owner = np.repeat(np.arange(2 * A, dtype=np.int64), np.repeat(n_a, 2))
        T, P, xe = (np.concatenate([np.tile(col[s], 2) for s in index]) for col in (Ts, Ps, xs))
        seg = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(n_a)])
        d = _upload(dev, [comp, kij, owner, T, P, xe, seg])
        x1, _, res, st = ops.pcsaft_kij_x1(d_params, d[0], d[1], None, d[2], d[3], d[4], d[5], d_feeds)
        return ops.pcsaft_kij_sums(res, x1, d[5], st, d[6], h).cpu().numpy()

    return evaluate, npts


def fit_kij(systems: Sequence[Any], feed_x1s: Optional[Any] = None, n: int = 50, k0: float = 0.2, diff_step: float = 1e-5,
            xtol: float = 1e-8, ftol: float = 1e-8, max_iter: int = 50) -> dict:
    """One k_12 per binary, fitted to measured liquid compositions by Levenberg-Marquardt on the residuals
    log((x1_pred + 1e-6) / (x1 + 1e-6)), all binaries in lockstep (the ``least_squares`` call of the reference's
    pcsaft/kij.py ``optimize_kij``, which fits one pair after the other).  ``systems``: a list of (parameters [2 rows],
    T [n_s] K, P [n_s] Pa, x1 [n_s]); ``feed_x1s``: the trial feeds of ``mix_kij_x1``, by default the reference's
    ``np.linspace(1e-5, 0.99, n)``.  Every iteration is one ``ops.pcsaft_kij_x1`` and one ``ops.pcsaft_kij_sums`` launch over
    the rows (k_trial, k_trial + diff_step) of the systems still active, and one download of [active, 8]; a system that has
    ended is in no later launch.  A point without a predicted x1 has the reference's penalty 10.0 as its residual and,
    unlike there, 0 as its derivative.  The forward difference is taken over ``diff_step`` = 1e-5, not scipy's 1.5e-8: the
    flash ends at 1e-10 in ln f.  -> the dict of ``_fit_kij_core``: [S] arrays ``k_12``, ``loss``, ``loss_nonan``, ``mape``,
    ``n_nan``, ``iterations``, ``reason``.  Liquid-liquid systems are not handled; no stability test runs (``mix_kij_x1``)."""
    feeds = np.linspace(1e-5, 0.99, int(n)) if feed_x1s is None else np.ascontiguousarray(feed_x1s, dtype=np.float64)
    if feeds.ndim != 1 or feeds.size == 0:
        raise ValueError(f"feed_x1s must be a non-empty 1-d array, got shape {feeds.shape}")
    if not (np.isfinite(diff_step) and diff_step != 0.0):
        raise ValueError(f"diff_step must be finite and not 0, got {diff_step}")
    evaluate, npts = _kij_evaluator(systems, feeds, diff_step)
    return _fit_kij_core(evaluate, npts, k0=k0, xtol=xtol, ftol=ftol, max_iter=max_iter)


def _kij_table(binary_vle: Any) -> List[Tuple[str, str, np.ndarray, np.ndarray, np.ndarray]]:
    """The VLE table of ``optimize_kij`` split by pair, on the host: (inchi1, inchi2, T_K, P_kPa, x1) of every pair in
    order of first appearance, rows with a null or NaN x1 dropped, pairs without a row left included (empty arrays).
    ``ValueError`` for a missing column or columns of unequal length."""
    missing = [c for c in KIJ_COLUMNS if c not in binary_vle]
    if missing:
        raise ValueError(f"binary_vle lacks the columns {missing}; it needs {list(KIJ_COLUMNS)}")
    cols = [list(binary_vle[c]) for c in KIJ_COLUMNS]
    if len({len(c) for c in cols}) != 1:
        raise ValueError(f"the columns of binary_vle differ in length: {[len(c) for c in cols]}")
    pairs: dict = {}
    for a, b, T, P, x in zip(*cols):
        rows = pairs.setdefault((a, b), [])
        if x is not None and not np.isnan(x):
            rows.append((np.nan if T is None else T, np.nan if P is None else P, x))
    out = []
    for (a, b), rows in pairs.items():
        t = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        out.append((a, b, t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()))
    return out


def _kij_co2_pressure_kpa(T: np.ndarray, vp_pa: np.ndarray) -> np.ndarray:
    """the pressure scale of the reference's CO2 check in kPa: ``vp_pa``, the CO2 vapour pressure at the T below 304.2 K in
    their order, there, and 7377.3 kPa elsewhere"""
    out = np.full(T.shape, _CO2_PC_KPA, dtype=np.float64)
    out[T < _CO2_TC] = np.asarray(vp_pa, dtype=np.float64) / 1e3
    return out


def optimize_kij(binary_vle: Any, inchi_to_params: Any, n: int = 50, co2_check: bool = True) -> dict:
    """The reference's pcsaft/kij.py ``optimize_kij``: one k_12 for every binary of a VLE table, all fitted at once by
    ``fit_kij``.  ``binary_vle`` is a mapping of column name to sequence (``polars.DataFrame.to_dict(as_series=False)``,
    ``pandas.DataFrame.to_dict("list")``) with the columns ``inchi1, inchi2, T_K, P_kPa, mole_fraction_c1p2``;
    ``inchi_to_params`` maps an InChI to its parameter row; ``n`` trial feeds ``np.linspace(1e-5, 0.99, n)``.  Rows with a
    null or NaN x1 are dropped and pairs are taken in order of first appearance.  With ``co2_check`` only rows with
    P_kPa / vp < 0.85 are kept, vp the CO2 vapour pressure (kPa) of ``inchi_to_params["InChI=1S/CO2/c2-1-3"]`` below
    304.2 K (one ``vp_batch`` launch for the whole table) and 7377.3 kPa from there on; ``KeyError`` without that key, as in
    the reference.  Pairs left without rows are skipped.  -> a dict of lists under the reference's keys ``inchi1, inchi2,
    k_12, loss, loss_nonan, mape, n_nan`` (``polars.DataFrame(result)`` is the reference's return value)."""
    table = _kij_table(binary_vle)
    co2 = inchi_to_params[CO2_INCHI] if co2_check else None
    unknown = sorted({c for a, b, *_ in table for c in (a, b) if c not in inchi_to_params})
    if unknown:
        raise KeyError(f"inchi_to_params has no parameters for {unknown}")  # before any launch
    if co2_check and table:
        T_all = np.concatenate([t[2] for t in table])
        cold = T_all[T_all < _CO2_TC]
        vp = vp_batch([co2], [cold[:, None]])[0] if cold.size else np.zeros(0)
        keep = np.concatenate([t[3] for t in table]) / _kij_co2_pressure_kpa(T_all, vp) < 0.85
        cuts = np.cumsum([t[2].size for t in table])[:-1]
        table = [(a, b, T[m], P[m], x[m]) for (a, b, T, P, x), m in zip(table, np.split(keep, cuts))]
    table = [t for t in table if t[2].size]
    out: dict = {key: [] for key in KIJ_KEYS}
    if not table:
        return out
    fit = fit_kij([([inchi_to_params[a], inchi_to_params[b]], T, P * 1e3, x) for a, b, T, P, x in table], n=n)
    out["inchi1"] = [t[0] for t in table]
    out["inchi2"] = [t[1] for t in table]
    for key in KIJ_KEYS[2:]:
        out[key] = fit[key].tolist()
    return out
