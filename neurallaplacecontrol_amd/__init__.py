"""neurallaplacecontrol_amd -- the Neural-Laplace-Control planning hot path on AMD MI355X (gfx950).

Drop-in mirrors of the reference's Python interfaces for this path:

    from neurallaplacecontrol_amd import MPPIDelay              # planners/mppi_delay.py:54
    from neurallaplacecontrol_amd import NeuralLaplaceModel     # w_nl.py:66
    from neurallaplacecontrol_amd import laplace_reconstruct    # torchlaplace (external)
    from neurallaplacecontrol_amd import NLTrainer              # train_utils.py:388-408 (fused training step)
    from neurallaplacecontrol_amd import DeltaTRNN, NODE        # train_utils.py:589, :664 (baseline models)
    from neurallaplacecontrol_amd import collect_expert_dataset # mppi_dataset_collector.py:324-443 (expert dataset)
    from neurallaplacecontrol_amd import generate_synthetic_dataset  # overlay.py:664-737 (synthetic dataset)

All arithmetic runs in hand-written HIP kernels behind the C ABI of ``libnlc_hip.so``
(``include/nlc.h``); importing the package does not touch the GPU.  There is no CPU fallback.
"""

from ._lib import set_default_options  # noqa: F401
from .envs import EnvCost, NLDynamics, OracleDynamics, initial_state, noise_sigma  # noqa: F401
from .collector import ExpertCollector, collect_expert_dataset, replay_buffer_file_name  # noqa: F401
from .env_loop import BatchedEnv, evaluate_episodes  # noqa: F401
from .laplace import ilt_reconstruct, laplace_reconstruct, rep_func_inputs  # noqa: F401
from .nl_model import LaplaceRepresentationFunc, NeuralLaplaceModel, ReverseGRUEncoder  # noqa: F401
from .node_model import NODE, xOdeFuncInXAndU  # noqa: F401
from .rnn_model import RNN, DeltaTRNN  # noqa: F401
from .training import (NLTrainer, NLTrainerGroup, NODETrainer, NODETrainerGroup, RNNTrainer,  # noqa: F401
                       RNNTrainerGroup)
from .synthetic import generate_synthetic_dataset, synthetic_dataset_shape  # noqa: F401
from .planners.mppi_batch import BatchedMPPIDelay  # noqa: F401
from .planners.mppi_delay import MPPIDelay  # noqa: F401

__all__ = [
    "MPPIDelay",
    "BatchedMPPIDelay",
    "BatchedEnv",
    "evaluate_episodes",
    "ExpertCollector",
    "collect_expert_dataset",
    "replay_buffer_file_name",
    "generate_synthetic_dataset",
    "synthetic_dataset_shape",
    "NeuralLaplaceModel",
    "NLTrainer",
    "NLTrainerGroup",
    "NODETrainer",
    "NODETrainerGroup",
    "RNNTrainer",
    "RNNTrainerGroup",
    "DeltaTRNN",
    "RNN",
    "NODE",
    "ReverseGRUEncoder",
    "LaplaceRepresentationFunc",
    "laplace_reconstruct",
    "ilt_reconstruct",
    "rep_func_inputs",
    "NLDynamics",
    "OracleDynamics",
    "EnvCost",
    "noise_sigma",
    "initial_state",
    "set_default_options",
]
