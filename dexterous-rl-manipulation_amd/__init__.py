"""dexterous-rl-manipulation_amd -- MI355X-native hot path of I2S9/dexterous-rl-manipulation.

Drop-in surfaces (same names as the reference modules):
  envs.DexterousManipulationEnv, rewards.{RewardShaping,SparseReward},
  policies.{SimpleLearner,RandomPolicy,HeuristicPolicy}, training.{run_episode,run_training_episode},
  experiments.{CurriculumConfig,CurriculumScheduler,StepBasedScheduler,ExperimentConfig,load_config,...},
  evaluation.{HeldOutObjectSet,CombinedNoiseWrapper,Evaluator,RobustnessTester,EvaluationMetrics,...},
  ablation.{train_with_config,run_component_ablation,...},
  curriculum_ablation.{train_with_curriculum,train_without_curriculum,compute_convergence_metrics,run_ablation_study},
  seed_variance.{SeedVarianceAnalyzer,analyze_seed_variance,plot_seed_variance,print_variance_report,run_seed_variance},
  failure_analysis.{print_failure_taxonomy,print_failure_statistics,analyze_failure_modes},
  failure_statistics.{load_failure_logs,compute_failure_distribution,compute_correlations,generate_failure_report,
                      plot_failure_distribution,plot_failure_correlations,run_failure_study},
  robustness_analysis.{analyze_robustness_results,plot_robustness_results,print_robustness_report,
                       run_robustness_study},
  reward_comparison.{run_training_comparison,compare_rewards}
Studies of the PG trainer (arms x seeds of fit(), reduced on the device): training_study.run_training_study,
  ablation.run_pg_component_study, curriculum_ablation.run_pg_curriculum_study, `python -m ...pg_ablation`.
Batched device API: envs.VecEnv, policies.VecSimpleLearner, training.SimpleLearnerRollout,
trainer.PGTrainer (iteration, fit, checkpoints; training_run.TrainingLog; `python -m ...train`).
The compute runs in libdxrl.so (HIP, gfx950; C ABI in include/dxrl.h).  No CPU fallback.
"""
from . import experiments, rewards  # noqa: F401  (no GPU needed to import)
from .experiments import CurriculumConfig  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    import importlib
    if name in ("envs", "policies", "training", "evaluation", "build", "_native", "trainer",
                "evaluator", "metrics", "curriculum_ablation", "seed_variance", "failure_analysis", "failure_statistics",
                "robustness_analysis", "training_run", "workloads", "reward_comparison", "ablation",
                "training_study", "pg_ablation"):
        return importlib.import_module(f".{name}", __name__)
    raise AttributeError(name)
