"""MI355X-native Crank-Nicolson finite-difference engine (fdcn).

Drop-in for the time-stepping hot path of rwx-gigaba-sonwabo/Finite_Difference:
the batched CN / Rannacher / knock-out / Ikonen-Toivanen march runs in HIP
kernels for gfx950 (libfdcn.so, C ABI in include/fdcn.h); the pricer façades
keep the reference's constructor arguments and methods.
"""
__version__ = "0.1.0"

from . import capi  # noqa: F401
from .engine import Engine, Solve, Boundary, default_engine  # noqa: F401
from .mc_barrier import (NacaCurve, BarrierSpec, RebateSpec, MCConfig,  # noqa: F401
                         price_discrete_barrier_mc, mc_barrier_batch, merge_mc_stats,
                         merge_qmc_stats)
from .bgk_barrier import DiscreteBarrierBGKPricer, bgk_price_batch  # noqa: F401
from .american_barrier import AmericanBarrierFDMPricer  # noqa: F401
from .american_knockin import AmericanKnockInFDMPricer  # noqa: F401
from .bermudan import BermudanFDMPricer  # noqa: F401
from .mc_american import (LsmContract, LsmConfig, plan_american_contract,  # noqa: F401
                          contract_from_pricer, simulate_lsm, price_american_mc,
                          mc_american_batch, merge_lsm_stats, DualConfig, simulate_dual,
                          mc_american_bounds_batch, price_american_mc_bounds,
                          merge_dual_stats, brackets)
