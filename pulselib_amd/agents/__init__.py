from .first_visit_mc import FirstVisitMonteCarlo
from .first_visit_mc_gpu import FirstVisitMonteCarloGPU
from .on_policy_first_visit_mc import OnPolicyFirstVisitMC
from .on_policy_first_visit_mc_gpu import OnPolicyFirstVisitMCGPU
from .qlearning import QLearningBatch
from .tfe_ntuple_td_gpu import NTupleTDAfterstateTFEGPU
from .tfe_on_policy_mc_gpu import OnPolicyFirstVisitMCTFEGPU

__all__ = ["FirstVisitMonteCarlo", "FirstVisitMonteCarloGPU", "NTupleTDAfterstateTFEGPU", "OnPolicyFirstVisitMC", "OnPolicyFirstVisitMCGPU", "OnPolicyFirstVisitMCTFEGPU",
           "QLearningBatch"]
