"""Pure-component PC-SAFT liquid density and vapour pressure on the GPU, for the validation metrics of
``GNNePCSAFTL.validation_step`` (``mape_den`` / ``mape_vp``).

Stands in for the reference's feos calls (gnnepcsaft/train/utils.py:238-300 ``rho_batch`` / ``vp_batch`` and
pcsaft/pcsaft_feos.py ``pure_den_feos`` / ``pure_vp_feos``), with the same arguments and results.  The arithmetic is
the fp64 kernel of csrc/gnx_pcsaft.hip; there is no CPU path.

Enable the native evaluation on a model with::

    from gnnepcsaft_amd import pcsaft
    model.rho_batch, model.vp_batch = pcsaft.rho_batch, pcsaft.vp_batch

Parameter rows are ``[m, sigma (Å), epsilon/k (K), kappa_ab, epsilon_ab/k (K), mu (D), na, nb, mw]``; state rows are
``[T (K), P (Pa), phase, tp, value]`` (only T and P are read).  Densities are in mol/m³, pressures in Pa.
"""
from __future__ import annotations

from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

STATUS_OK, STATUS_NO_CONVERGENCE, STATUS_SUPERCRITICAL, STATUS_BAD_INPUT = 0, 1, 2, 3
_REASON = {STATUS_NO_CONVERGENCE: "no root / not converged", STATUS_SUPERCRITICAL: "temperature at or above the "
           "critical temperature", STATUS_BAD_INPUT: "invalid parameters or state"}


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.GnxError(_lib.GNX_E_INVALID, "gnnepcsaft_amd.pcsaft needs a HIP device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _run(kind: str, params: np.ndarray, owner: np.ndarray, T: np.ndarray, P: Optional[np.ndarray]
         ) -> Tuple[np.ndarray, np.ndarray]:
    """One upload, one launch, one download: (value [n] fp64, status [n] int32) for host arrays."""
    B, n = params.shape[0], owner.shape[0]
    # every input in one 8-byte-element host buffer: params | T | P | owner
    buf = np.empty(9 * B + 3 * n, dtype=np.int64)
    flt = buf.view(np.float64)
    flt[:9 * B] = params.reshape(-1)
    flt[9 * B:9 * B + n] = T
    if P is not None:
        flt[9 * B + n:9 * B + 2 * n] = P
    buf[9 * B + 2 * n:] = owner
    dev = _device()
    dbuf = torch.from_numpy(buf).to(dev)
    dflt = dbuf.view(torch.float64)
    d_params, d_T, d_P, d_owner = dflt[:9 * B], dflt[9 * B:9 * B + n], dflt[9 * B + n:9 * B + 2 * n], dbuf[9 * B + 2 * n:]
    # both outputs in one buffer: value (fp64) | status (int32, padded to 8 bytes)
    out = torch.empty(n + (n + 1) // 2, dtype=torch.int64, device=dev)
    value, status = out[:n].view(torch.float64), out[n:].view(torch.int32)[:n]
    lib = _lib.load()
    if kind == "rho":
        _lib.check(lib.gnx_pcsaft_density(_lib.handle(dev), d_params.data_ptr(), B, d_owner.data_ptr(),
                                          d_T.data_ptr(), d_P.data_ptr(), n, value.data_ptr(), status.data_ptr()))
    else:
        _lib.check(lib.gnx_pcsaft_vapor_pressure(_lib.handle(dev), d_params.data_ptr(), B, d_owner.data_ptr(),
                                                 d_T.data_ptr(), n, value.data_ptr(), None, None, status.data_ptr()))
    host = out.cpu().numpy()
    return host[:n].view(np.float64).copy(), host[n:].view(np.int32)[:n].copy()


def _rows(parameters_batch: Sequence[Sequence[float]]) -> np.ndarray:
    params = np.asarray(parameters_batch, dtype=np.float64).reshape(-1, 9)
    if params.shape[0] != len(parameters_batch):
        raise ValueError(f"expected {len(parameters_batch)} parameter rows of 9 values, got {np.shape(parameters_batch)}")
    return params


def _batch(kind: str, parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    if len(parameters_batch) != len(states_batch):
        raise ValueError(f"{len(parameters_batch)} parameter rows but {len(states_batch)} state tables")
    tables = [(i, np.asarray(s, dtype=np.float64)) for i, s in enumerate(states_batch) if s.shape[0] > 0]
    if not tables:
        return []
    params = _rows(parameters_batch)
    owner = np.concatenate([np.full(t.shape[0], i, dtype=np.int64) for i, t in tables])
    states = np.concatenate([t.reshape(t.shape[0], -1) for _, t in tables])
    value, _ = _run(kind, params, owner, states[:, 0], states[:, 1] if kind == "rho" else None)
    cuts = np.cumsum([t.shape[0] for _, t in tables])[:-1]
    return [v.copy() for v in np.split(value, cuts)]


def rho_batch(parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    """Liquid densities (mol/m³) of every state of every non-empty table, one fp64 array per such table, 0.0 where a
    point failed (reference train/utils.py:252-268)."""
    return _batch("rho", parameters_batch, states_batch)


def vp_batch(parameters_batch: List[List[Any]], states_batch: List[Any]) -> List[np.ndarray]:
    """Vapour pressures (Pa) at the temperature of every state of every non-empty table, one fp64 array per such
    table, 0.0 where a point failed (reference train/utils.py:284-300)."""
    return _batch("vp", parameters_batch, states_batch)


def _single(kind: str, parameters: Sequence[float], state: Sequence[float]) -> float:
    params = _rows([parameters])
    P = np.asarray([state[1]], dtype=np.float64) if kind == "rho" else None
    value, status = _run(kind, params, np.zeros(1, dtype=np.int64), np.asarray([state[0]], dtype=np.float64), P)
    if status[0] != STATUS_OK:
        raise RuntimeError(f"PC-SAFT {'density' if kind == 'rho' else 'vapor pressure'} failed at state "
                           f"{list(state)}: {_REASON.get(int(status[0]), int(status[0]))}")
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
