"""antsrl_amd — MI355X-native AntsRL environment step loop (hand-written HIP behind the
reference's RLApi surface).  See DESIGN.md."""
from . import config  # noqa: F401
from .config import AntsCfg, make_cfg  # noqa: F401

__all__ = ["config", "AntsCfg", "make_cfg", "CollectAgent", "LinearTrainer", "ExploreAgent", "ExploreTrainer",
           "JointTrainer", "ReworkTrainer", "ReworkAgent", "EpisodeMonitor", "train_episodes", "epsilon_schedule", "EpisodeStats",
           "EnvCheckpoint", "PopulationAgent", "train_population", "PopulationExploreAgent", "train_population_curriculum",
           "PopulationJointAgent", "PopulationMemoryAgent", "PopulationReworkAgent", "PopulationFitness", "PbtConfig",
           "pbt_plan"]


def __getattr__(name):  # the linear agent and its trainer import torch: resolved on first use
    if name == "CollectAgent":
        from .agent import CollectAgent
        return CollectAgent
    if name == "LinearTrainer":
        from .train import LinearTrainer
        return LinearTrainer
    if name == "ExploreAgent":
        from .agent import ExploreAgent
        return ExploreAgent
    if name == "ExploreTrainer":
        from .train import ExploreTrainer
        return ExploreTrainer
    if name == "JointTrainer":
        from .train import JointTrainer
        return JointTrainer
    if name == "ReworkTrainer":
        from .train import ReworkTrainer
        return ReworkTrainer
    if name == "ReworkAgent":
        from .agent import ReworkAgent
        return ReworkAgent
    if name == "EpisodeMonitor":
        from .monitor import EpisodeMonitor
        return EpisodeMonitor
    if name == "EpisodeStats":
        from .stats import EpisodeStats
        return EpisodeStats
    if name == "EnvCheckpoint":
        from .checkpoint import EnvCheckpoint
        return EnvCheckpoint
    if name in ("PopulationAgent", "PopulationExploreAgent", "PopulationJointAgent", "PopulationMemoryAgent",
                "PopulationReworkAgent"):
        from . import population
        return getattr(population, name)
    if name in ("PopulationFitness", "PbtConfig", "pbt_plan"):
        from . import pbt
        return getattr(pbt, name)
    if name in ("train_episodes", "train_population", "train_population_curriculum", "epsilon_schedule"):
        from . import driver
        return getattr(driver, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
