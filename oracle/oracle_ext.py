"""ctypes loader for the REAL-typed plan solvers (oracle/fdcn_oracle_ext.c).

TEST INFRASTRUCTURE ONLY, under the rule of oracle.py's header: importable by
tests/ as the checker; the product package never imports it.

Builds of one source, selected by ``kind``:
  "f64"     double, -ffp-contract=off: bit-identical to oracle.cn_batch/it_batch
  "f64fma"  double, contracted a*b+c (needs a CPU with FMA)
  "ld"      long double (64-bit significand on x86): the tests' reference
  "quad"    __float128; optional (`make -C oracle quad`), see quad_available()
  "f64conv", "ldconv"  the march kernels' ordering of the solve (converged LU +
            Sherman-Morrison), sequential, in double (contracted) / long double
  "f64rec", "ldrec"    the same with the Crank-Nicolson right-hand side
            recovered from the previous step's (the kernels' split/recovery forms)

Every entry returns (hi, lo), two fp64 arrays with x = hi + lo, hi = (double)x.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Dict, Tuple

import numpy as np

from .oracle import HERE, _PD, _PI32, _I32, _f64, _i32, _pd

KINDS = ("f64", "f64fma", "ld", "quad", "f64conv", "ldconv", "f64rec", "ldrec")
_libs: Dict[str, ctypes.CDLL] = {}


def lib_path(kind: str) -> str:
    return os.path.join(HERE, "build", f"liboracle_ext_{kind}.so")


def _cpu_has_fma() -> bool:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    return " fma " in line + " "
    except OSError:
        pass
    return True


def quad_available() -> bool:
    """Build the optional __float128 library if it is not there; False where
    the toolchain has no libquadmath."""
    if os.path.exists(lib_path("quad")):
        return True
    r = subprocess.run(["make", "-s", "-C", HERE, "quad"], stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
    return r.returncode == 0 and os.path.exists(lib_path("quad"))


def lib(kind: str) -> ctypes.CDLL:
    if kind not in KINDS:
        raise ValueError(kind)
    L = _libs.get(kind)
    if L is None:
        if kind == "quad":
            if not quad_available():
                raise RuntimeError("liboracle_ext_quad.so cannot be built (libquadmath)")
        else:
            # make is a no-op when the library is newer than its source
            subprocess.run(["make", "-s", "-C", HERE], check=True)
        if kind in ("f64fma", "f64conv", "f64rec") and not _cpu_has_fma():
            raise RuntimeError(f"the {kind} realisation needs a CPU with FMA")
        L = ctypes.CDLL(lib_path(kind))
        L.oracle_ext_cn_batch.restype = ctypes.c_int
        L.oracle_ext_cn_batch.argtypes = [_I32, _I32, _I32, _I32, _PD, _PI32, _PD, _I32, _PI32,
                                          _PD, _PD, _PD, _I32]
        L.oracle_ext_it_batch.restype = ctypes.c_int
        L.oracle_ext_it_batch.argtypes = [_I32, _I32, _I32, _I32, _PD, _PI32, _PD, _PD, _PD, _PD,
                                          _I32]
        L.oracle_ext_vc_batch.restype = ctypes.c_int
        L.oracle_ext_vc_batch.argtypes = [_I32, _I32, _I32, _I32, _PD, _PD, _PD, _PI32, _I32,
                                          _PI32, _PD, _PD, _PD, _I32, _I32]
        L.oracle_ext_mant_dig.restype = ctypes.c_int
        _libs[kind] = L
    return L


def mant_dig(kind: str) -> int:
    return int(lib(kind).oracle_ext_mant_dig())


def cn_batch(kind: str, n_nodes: int, n_time: int, n_ranna: int, params, iparams, v_init,
             mon_step, mon_rebate, nthreads: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    P, I, V = _f64(params), _i32(iparams), _f64(v_init)
    B = V.shape[0]
    ms = _i32(mon_step) if len(mon_step) else _i32([0])
    mr = _f64(mon_rebate) if len(mon_rebate) else _f64([0.0])
    hi = np.empty((B, n_nodes), dtype=np.float64)
    lo = np.empty((B, n_nodes), dtype=np.float64)
    rc = lib(kind).oracle_ext_cn_batch(B, n_nodes, n_time, n_ranna, _pd(P),
                                       I.ctypes.data_as(_PI32), _pd(V), len(mon_step),
                                       ms.ctypes.data_as(_PI32), _pd(mr), _pd(hi), _pd(lo),
                                       int(nthreads))
    if rc != 0:
        raise RuntimeError(f"oracle_ext_cn_batch[{kind}] failed ({rc})")
    return hi, lo


VC_THOMAS, VC_KERNEL_STENCIL, VC_KERNEL_POINTWISE = 0, 1, 2


def vc_batch(kind: str, n_nodes: int, n_time: int, n_ranna: int, diag, bnd, v_init, iparams,
             mon_step, mon_rebate, nthreads: int = 1,
             order: int = VC_THOMAS) -> Tuple[np.ndarray, np.ndarray]:
    """The spot-space per-row march on the fdcn_vc_batch plan (oracle.vc_batch's
    arguments) in the arithmetic `kind` ("f64", "f64fma", "ld", "quad").
    order: the Thomas march, or the sequential restatement of fdcn_vc.hip's
    ordering in its stencil / pointwise form."""
    D, Bd, V, I = _f64(diag), _f64(bnd), _f64(v_init), _i32(iparams)
    B = V.shape[0]
    ms = _i32(mon_step) if len(mon_step) else _i32([0])
    mr = _f64(mon_rebate) if len(mon_rebate) else _f64([0.0])
    if Bd.size == 0:
        Bd = _f64([0.0, 0.0])
    hi = np.empty((B, n_nodes), dtype=np.float64)
    lo = np.empty((B, n_nodes), dtype=np.float64)
    rc = lib(kind).oracle_ext_vc_batch(B, n_nodes, n_time, n_ranna, _pd(D), _pd(Bd), _pd(V),
                                       I.ctypes.data_as(_PI32), len(mon_step),
                                       ms.ctypes.data_as(_PI32), _pd(mr), _pd(hi), _pd(lo),
                                       int(order), int(nthreads))
    if rc != 0:
        raise RuntimeError(f"oracle_ext_vc_batch[{kind}] failed ({rc})")
    return hi, lo


def it_batch(kind: str, n_nodes: int, n_time: int, n_ranna: int, params, iparams, v_init,
             payoff, nthreads: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    P, I, V, F = _f64(params), _i32(iparams), _f64(v_init), _f64(payoff)
    B = V.shape[0]
    hi = np.empty((B, n_nodes), dtype=np.float64)
    lo = np.empty((B, n_nodes), dtype=np.float64)
    rc = lib(kind).oracle_ext_it_batch(B, n_nodes, n_time, n_ranna, _pd(P),
                                       I.ctypes.data_as(_PI32), _pd(V), _pd(F), _pd(hi),
                                       _pd(lo), int(nthreads))
    if rc != 0:
        raise RuntimeError(f"oracle_ext_it_batch[{kind}] failed ({rc})")
    return hi, lo
