"""ldsr_amd -- MI355X-native engine for ldsr's EM/Kalman restart path.

Only the hot path lives here: the HIP kernels + C ABI (csrc/, include/ldsr_hip.h) and the
host-side mirror of the reference's operator interface (api.py; sim.py: LDS_rep; ga.py: LDS_GA; bfgs.py: LDS_BFGS; pcr.py: the benchmark model R/PCR.R;
filter.py: the Kalman filter's outputs and the innovation diagnostics)."""
from .api import (ALGO_AUTO, ALGO_PAIR, ALGO_QUAD, ALGO_SCAN, ALGO_SERIAL, Kalman_smoother, LDS_EM,  # noqa: F401
                  LDS_EM_restart, Mstep, em_batch, em_restart_grid, ensemble_restart, make_init, pack_theta, penalized_likelihood,
                  propagate,
                  select_restart, smooth_batch, unpack_theta)
from .sim import LDS_rep, one_LDS_rep, simulate_batch  # noqa: F401,E402
from .ga import LDS_GA, ga_batch  # noqa: F401,E402
from .bfgs import LDS_BFGS, LDS_BFGS_with_update, bfgs_batch, bfgs_update_batch, pl_grad, ssq_train  # noqa: F401,E402
from .pcr import PCR_ensemble_selection, PCR_reconstruction, cvPCR, one_pcr_cv, pcr_batch  # noqa: F401,E402
from .filter import Kalman_filter, filter_batch, innovation_diagnostics  # noqa: F401,E402
from . import bfgs, cv, filter, ga, pcr, shard, sim  # noqa: F401,E402
