"""Failure analysis and reporting -- evaluation/failure_analysis.py:11-99.

Same names, signatures, result dictionaries and printed text as the reference, on
``failures.FailureClassifier`` (the classifier goes through the same NumPy calls on
the same lists, so modes and confidences are the reference's).  The descriptions and
indicator lists ``print_failure_taxonomy`` prints are this package's own wording of
the taxonomy (failures.FAILURE_MODE_DEFINITIONS); the layout is the reference's.

The device form of the same analysis -- no per-episode data on the host -- is
``failure_statistics.run_failure_study``.
"""
from __future__ import annotations

from typing import Dict, List

from .failures import FAILURE_MODE_DEFINITIONS, FailureClassifier

_BAR = "=" * 60


def print_failure_taxonomy():
    """failure_analysis.py:11-24."""
    print(_BAR)
    print("Dexterous Manipulation Failure Taxonomy")
    print(_BAR)
    for mode, definition in FAILURE_MODE_DEFINITIONS.items():
        print(f"\n{mode.value.upper()}: {definition.name}")
        print(f"  Description: {definition.description}")
        print("  Key Indicators:")
        for indicator in definition.key_indicators:
            print(f"    - {indicator}")
    print("\n" + _BAR)


def print_failure_statistics(statistics: Dict):
    """failure_analysis.py:27-58: totals, then the modes by descending frequency."""
    print("\n" + _BAR)
    print("Failure Mode Statistics")
    print(_BAR)
    print("\nOverall:")
    print(f"  Total episodes: {statistics['total_episodes']}")
    print(f"  Successful: {statistics['successful_episodes']} ({statistics['success_rate']:.1%})")
    print(f"  Failed: {statistics['failed_episodes']}")
    print("\nFailure Mode Distribution:")
    counts = statistics["failure_counts"]
    for mode, frequency in sorted(statistics["failure_frequencies"].items(), key=lambda x: x[1], reverse=True):
        print(f"  {mode}: {counts[mode]} episodes ({frequency:.1%})")
    print(_BAR)


def analyze_failure_modes(episodes: List[Dict], max_steps: int = 200, success_threshold: int = 3) -> Dict:
    """failure_analysis.py:61-99: the classifier's statistics plus, per failure mode that
    occurred, its count, mean episode length, mean contact count and episodes."""
    statistics = FailureClassifier(success_threshold=success_threshold).get_failure_statistics(episodes, max_steps)
    detailed = {}
    for mode, eps in statistics["classified_episodes"].items():
        if mode is None or len(eps) == 0:
            continue
        lengths = [e["episode_steps"] for e in eps]
        contacts = [e.get("num_contacts", 0) for e in eps]
        detailed[mode.value] = {"count": len(eps),
                                "mean_episode_length": float(sum(lengths) / len(lengths)) if lengths else 0.0,
                                "mean_contacts": float(sum(contacts) / len(contacts)) if contacts else 0.0,
                                "episodes": eps}
    statistics["detailed_analysis"] = detailed
    return statistics


__all__ = ["print_failure_taxonomy", "print_failure_statistics", "analyze_failure_modes"]
