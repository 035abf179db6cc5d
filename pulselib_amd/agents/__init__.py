from .first_visit_mc import FirstVisitMonteCarlo
from .first_visit_mc_gpu import FirstVisitMonteCarloGPU
from .qlearning import QLearningBatch

__all__ = ["FirstVisitMonteCarlo", "FirstVisitMonteCarloGPU", "QLearningBatch"]
