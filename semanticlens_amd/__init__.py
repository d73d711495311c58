"""semanticlens_amd — the SemanticLens concept-database hot path on AMD MI355X (gfx950).

Drop-in for ``semanticlens`` (jim-berend/semanticlens v0.2.1) on that path: the same
``Lens`` / ``ActivationComponentVisualizer`` / ``foundation_models`` / ``scores`` API
(reference ``semanticlens/__init__.py:35-47``) over hand-written HIP kernels reached through
the C ABI in ``include/semanticlens_amd.h``.  No CPU fallback: without the built library and a
HIP device, compute calls raise.
"""
from __future__ import annotations

from semanticlens_amd import foundation_models, scores, utils
from semanticlens_amd.lens import (ConceptAudit, ConceptDBComparison, Decomposition, HubnessLabels, LabelDistribution, LabelRanks, Lens,
                                   audit_concepts, compare_concept_dbs, decompose_components, label_components_csls,
                                   label_distribution, label_facets, label_rank, probe_csls, probe_decompose, probe_rank,
                                   probe_setmax, probe_softmax, search_facets)
from semanticlens_amd.scores import (Facets, RedundancyGroups, clarity_score, polysemanticity_facets, polysemanticity_score,
                                     redundancy_groups, redundancy_score, silhouette_samples, silhouette_score)

__version__ = "0.1.0"

__all__ = [
    "foundation_models",
    "scores",
    "utils",
    "Lens",
    "compare_concept_dbs",
    "ConceptDBComparison",
    "audit_concepts",
    "ConceptAudit",
    "probe_setmax",
    "label_distribution",
    "LabelDistribution",
    "probe_softmax",
    "label_rank",
    "LabelRanks",
    "probe_rank",
    "decompose_components",
    "Decomposition",
    "probe_decompose",
    "label_components_csls",
    "HubnessLabels",
    "probe_csls",
    "clarity_score",
    "polysemanticity_score",
    "redundancy_score",
    "redundancy_groups",
    "RedundancyGroups",
    "Facets",
    "polysemanticity_facets",
    "label_facets",
    "search_facets",
    "silhouette_samples",
    "silhouette_score",
]
