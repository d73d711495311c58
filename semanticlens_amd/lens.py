"""Lens — orchestration of concept-DB build, probing and evaluation.

Mirror of ``semanticlens/lens.py`` (reference v0.2.1): same module-level functions and ``Lens``
methods, same cache-file naming.  Text/image probing runs the template-difference mean (K10)
and the cosine GEMM (K6) on the device; query embeddings are not bounced through the host
between the text tower and the GEMM.
"""
from __future__ import annotations

import os

import logging
import operator
from collections.abc import Mapping
from dataclasses import dataclass

import torch
from safetensors.torch import load_file, save_file
from tqdm.auto import tqdm

from semanticlens_amd import _native as N
from semanticlens_amd.component_visualization.base import AbstractComponentVisualizer
from semanticlens_amd.foundation_models.base import AbstractVLM
from semanticlens_amd.scores import (Facets, clarity_score, polysemanticity_facets, polysemanticity_score, redundancy_groups,
                                     redundancy_score, similarity_score)
from semanticlens_amd.utils.helper import get_fallback_name

logger = logging.getLogger(__name__)


def compute_concept_db(cv: AbstractComponentVisualizer, fm: AbstractVLM, **kwargs):
    """Stateless concept-DB build: delegates to ``cv._compute_concept_db(fm, **kwargs)`` (lens.py:27-56)."""
    return cv._compute_concept_db(fm, **kwargs)


def text_probing(fm, query, aggregated_concept_db, templates=None, batch_size=None):
    """Cosine similarity of text queries against ``(n_components, D)`` concept embeddings (lens.py:59-121)."""
    queries = query if isinstance(query, list) else [query]
    query_embeds = _embed_text_probes(fm, queries, templates, batch_size)
    assert query_embeds.ndim == 2
    assert query_embeds.shape[0] == len(queries)
    return _probe(query_embeds, aggregated_concept_db)


def image_probing(fm, query, aggregated_concept_db):
    """Cosine similarity of an image query (several images are averaged) against the DB (lens.py:124-162)."""
    return _probe(_embed_image_probe(fm, query), aggregated_concept_db)


@torch.no_grad()
def _embed_image_probe(fm, query) -> torch.Tensor:
    """``(1, D)`` probe vector of one image or of a list of images (lens.py:158-160).

    Several images are averaged on the HOST, as the reference does (it moves the ``(n_images, D)`` embeddings to the
    CPU first): torch's device ``mean`` multiplies by a reciprocal where the CPU one divides, which differs in the last
    bit; the tensor is a few KB."""
    embeds = fm.encode_image(fm.preprocess(query).to(fm.device))
    if embeds.shape[0] > 1:
        return embeds.cpu().mean(0)[None]
    return embeds


def _encode_texts(fm, texts: list[str], batch_size: int | None = None, progress: bool = False):
    """``fm.encode_text(fm.tokenize(chunk))`` over ``texts`` in chunks of ``batch_size`` (lens.py:176-191).

    With several chunks the tokenizer (host Python: 6-9 ms per 1 024 prompts for the bench's stand-in, more for a BPE) runs one
    chunk AHEAD on a helper thread while the device encodes the current one — the text tower waits on a readback per batch, which
    releases the GIL — so a 10 000-prompt probe costs max(tokenise, encode) instead of their sum.  Same calls, same order, same
    results; ``SL_TEXT_PREFETCH=0`` restores the serial loop."""
    batch_size = batch_size or len(texts)
    starts = list(range(0, len(texts), batch_size))
    chunks = []
    bar = tqdm(starts, desc="text embedding ...", leave=False, disable=not progress or batch_size >= len(texts))
    if len(starts) > 1 and os.environ.get("SL_TEXT_PREFETCH", "1") != "0":
        from concurrent.futures import ThreadPoolExecutor

        # A new thread's current HIP device is 0 and its current stream the default one.  A wrapper's `tokenize` may end in
        # `.to(self.device)`: with an index-less device ("cuda") that copy would land on GPU 0 on every rank, issued on a stream
        # the encoder does not run on.  The helper therefore tokenises under the CALLER's device and stream; `.to(fm.device)` on
        # the main thread is then a no-op for tensors already there.
        dev = torch.device(fm.device)
        if dev.type == "cuda":
            cur_dev = torch.cuda.current_device() if dev.index is None else dev.index
            cur_stream = torch.cuda.current_stream(cur_dev)

            def tokenize(chunk):
                with torch.cuda.device(cur_dev), torch.cuda.stream(cur_stream):
                    return fm.tokenize(chunk)
        else:
            tokenize = fm.tokenize
        with ThreadPoolExecutor(max_workers=1) as pool:
            nxt = pool.submit(tokenize, texts[starts[0] : starts[0] + batch_size])
            for i, _ in enumerate(bar):
                tokens = nxt.result()
                if i + 1 < len(starts):
                    nxt = pool.submit(tokenize, texts[starts[i + 1] : starts[i + 1] + batch_size])
                chunks.append(fm.encode_text(tokens.to(fm.device)))
    else:
        for start in bar:
            chunks.append(fm.encode_text(fm.tokenize(texts[start : start + batch_size]).to(fm.device)))
    return chunks[0] if len(chunks) == 1 else torch.cat(chunks, dim=0)


@torch.no_grad()
def _embed_text_probes(fm, query: list[str], templates: list[str] | None, batch_size: int | None, encode=None):
    """Tokenise + encode the (templated) queries; with templates, subtract the empty-template
    embedding and average over templates (lens.py:165-203).

    The reference builds the templated list template-major (``for t in templates for q in query``,
    :174) but regroups it query-major (``"(q t) d -> q t d"``, :197).  That grouping is kept
    (SURVEY.md finding 4) so probing scores equal the reference's.

    ``encode(texts, batch_size)`` replaces the local text tower (``distributed.text_probing_sharded`` shards the
    prompt list across ranks there); each prompt's embedding does not depend on how the list is split.
    """
    if templates:
        query_templated = [t.format(q) for t in templates for q in query]
        empty_templates = [t.format("") for t in templates]
        if encode is None:
            templated = _encode_texts(fm, query_templated, batch_size, progress=True)
        else:
            templated = encode(query_templated, batch_size)
        empty = fm.encode_text(fm.tokenize(empty_templates).to(fm.device))
        return N.template_mean(templated, empty, len(query))
    if encode is not None:
        return encode(query, None)
    return fm.encode_text(fm.tokenize(query).to(fm.device))


@torch.no_grad()
def _probe(query: torch.Tensor, aggregated_concept_db):
    if isinstance(aggregated_concept_db, torch.Tensor):
        return similarity_score(query.to(aggregated_concept_db.device), aggregated_concept_db)
    keys = list(aggregated_concept_db)
    values = [aggregated_concept_db[k] for k in keys]
    # all layers in one native call (query normalised + split once) when none of them hits a shape quirk
    if values and all(isinstance(v, torch.Tensor) for v in values) and len({v.device for v in values}) == 1:
        outs = N.similarity_multi(query, values)
        if outs is not None:
            return {k: o.to(v.device) for k, o, v in zip(keys, outs, values)}
    return {key: similarity_score(query.to(value.device), value) for key, value in aggregated_concept_db.items()}


# ------------------------------------------------------------------------------------------------
# describe / search: top-k cosine without the full matrix (K6 tiles + K17 selection)
# ------------------------------------------------------------------------------------------------
LABEL_CHUNK_WORDS = 8192  # vocabulary words embedded and probed at a time when ``chunk_size`` is not given


def _db_layers(aggregated_concept_db):
    """``(names, tensors, is_dict)`` of a ``(C, D)`` tensor or a dict of them; shape errors raise before the device is touched."""
    is_dict = not isinstance(aggregated_concept_db, torch.Tensor)
    names = list(aggregated_concept_db) if is_dict else [None]
    layers = [aggregated_concept_db[n] for n in names] if is_dict else [aggregated_concept_db]
    for name, layer in zip(names, layers):
        if not isinstance(layer, torch.Tensor) or layer.ndim != 2:
            what = f"layer {name!r}" if is_dict else "the concept DB"
            raise ValueError(f"{what} must be a 2-D (n_components, D) tensor, got {tuple(getattr(layer, 'shape', ()))}")
    widths = {layer.shape[1] for layer in layers}
    if len(widths) > 1:
        raise ValueError(f"the layers' embedding widths differ: {sorted(widths)}")
    return names, layers, is_dict


def _check_width(embeds: torch.Tensor, layers):
    if embeds.ndim != 2:
        raise ValueError(f"query embeddings must be 2-D (n, D), got {tuple(embeds.shape)}")
    if layers and embeds.shape[1] != layers[0].shape[1]:
        raise ValueError(f"embedding width {embeds.shape[1]} does not match the concept DB's {layers[0].shape[1]}")


@torch.no_grad()
def _embed_words(fm, words: list[str], templates: list[str] | None, batch_size: int | None, empty=None) -> torch.Tensor:
    """``(len(words), D)`` text embeddings; with templates, each word's mean over ITS OWN templates minus the empty-template
    embedding.  The templated list is built query-major (``for w in words for t in templates``), the grouping
    ``N.template_mean`` reads (``E[(q * T + t) * D + d]``) — unlike ``_embed_text_probes``, whose template-major list regrouped
    query-major mixes the queries of one call (kept there because the reference does it).  ``empty``: the ``(T, D)``
    empty-template embeddings when the caller already has them."""
    if not templates:
        return _encode_texts(fm, words, batch_size)
    templated = _encode_texts(fm, [t.format(w) for w in words for t in templates], batch_size)
    if empty is None:
        empty = fm.encode_text(fm.tokenize([t.format("") for t in templates]).to(fm.device))
    return N.template_mean(templated, empty, len(words))


def _embedded_chunks(fm, texts: list[str], layers, templates: list[str] | None, batch_size: int | None, chunk_size: int | None):
    """``(start, stop, embeds)`` for ``texts`` embedded ``chunk_size`` (default ``LABEL_CHUNK_WORDS``) at a time, each chunk checked against
    the DB's width.  The call checks ``chunk_size``; the text tower (empty templates first) only runs when the result is iterated."""
    if chunk_size is not None and chunk_size < 1:
        raise ValueError(f"chunk_size = {chunk_size} must be at least 1")
    step = chunk_size or LABEL_CHUNK_WORDS
    def chunks():
        empty = fm.encode_text(fm.tokenize([t.format("") for t in templates]).to(fm.device)) if templates else None
        for start in range(0, len(texts), step):
            stop = min(start + step, len(texts))
            embeds = _embed_words(fm, texts[start:stop], templates, batch_size, empty)
            _check_width(embeds, layers)
            yield start, stop, embeds

    return chunks()


def _embed_vocabulary(fm, vocabulary: list[str], layers, templates: list[str] | None, batch_size: int | None,
                      chunk_size: int | None) -> torch.Tensor:
    """The whole vocabulary as ONE resident ``(V, D)`` fp32 device tensor, embedded ``chunk_size`` words at a time exactly as
    ``label_components`` embeds it (``_embedded_chunks``: ``chunk_size`` is checked by the call, before the text tower runs).  For
    the callers that revisit every word after having seen them all (``decompose_components``, ``label_components_csls``)."""
    chunks = _embedded_chunks(fm, vocabulary, layers, templates, batch_size, chunk_size)
    if layers:
        N._f32c(layers[0][:0])  # raises without a HIP device, before the text tower runs
    w = None
    for start, stop, embeds in chunks:
        if w is None:
            w = torch.empty((len(vocabulary), embeds.shape[1]), dtype=torch.float32, device=N.to_device(embeds).device)
        w[start:stop] = embeds
    return w


def _probe_layers(names, layers, is_dict, query_embeds: torch.Tensor, probe):
    """``probe(layer, queries) -> (values, ids)`` per layer, both operands on the layer's device as contiguous fp32 (the queries
    move only when the device changes); results on the device the layer came from, a dict of them for a dict DB."""
    out, q = {}, None
    for name, layer in zip(names, layers):
        ld = N._f32c(layer)
        q = N._f32c(query_embeds, ld.device) if q is None or q.device != ld.device else q
        out[name] = tuple(t.to(layer.device) for t in probe(ld, q))
    return out if is_dict else out[None]


def _decode_layers(ids: torch.Tensor, sizes: list[int]):
    """Global component ids (``offset[layer] + component``; -1 = empty slot) -> ``(layer_index, component)``."""
    ends = torch.tensor(sizes, dtype=torch.int64, device=ids.device).cumsum(0)
    layer = torch.bucketize(ids, ends, right=True)
    component = ids - (ends - torch.tensor(sizes, dtype=torch.int64, device=ids.device))[layer.clamp(max=len(sizes) - 1)]
    empty = ids < 0
    return layer.masked_fill(empty, -1), component.masked_fill(empty, -1)


@torch.no_grad()
def probe_topk(query_embeds: torch.Tensor, aggregated_concept_db, k: int, per: str = "component", chunk_rows: int | None = None):
    """Top-``k`` cosine between ``query_embeds (Q, D)`` and a concept DB (a ``(C, D)`` tensor or a dict of layers), for
    callers who bring their own vectors (an image vocabulary, say).  The ``(Q, C)`` matrix is never formed: the cosine GEMM
    writes one tile at a time and the streaming fp32 top-k (K17) folds it into a ``(rows, k)`` state.

    * ``per="component"``: for every component its best queries — ``(values (C, k) float32, ids (C, k) int64)`` with ``ids``
      indexing ``query_embeds``, or a dict of such pairs for a dict DB.
    * ``per="query"``: for every query its best components ACROSS all layers — ``(values (Q, k), layer_index (Q, k),
      component (Q, k), layer_names)``; per layer a top-k over the layer's components under the global id
      ``offset[layer] + component``, then a merge of the layers' states.  ``layer_names`` is ``[None]`` for a tensor DB.

    Order: larger cosine first, NaN before every number, equal cosines by the smaller id.  Slots beyond the number of
    candidates hold ``-inf`` / ``-1``.  Always ``normalize(x) @ normalize(y).T``: none of ``similarity_score``'s shape
    branches apply.  Results live on the DB's device (its first layer's for ``per="query"``)."""
    k = N.check_topk_k(k)
    if per not in ("component", "query"):
        raise ValueError(f'per must be "component" or "query", got {per!r}')
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    _check_width(query_embeds, layers)
    if per == "component":
        return _probe_layers(names, layers, is_dict, query_embeds, lambda ld, q: N.topk_probe(ld, q, k, chunk_rows))
    q = N._f32c(query_embeds)
    vals, ids = N.topk_new(q.shape[0], k, q.device)
    offset = 0
    for layer in layers:
        lv, li = N.topk_probe(q, N._f32c(layer, q.device), k, chunk_rows, id_base=offset)
        N.topk_merge_states(vals, ids, lv, li)
        offset += layer.shape[0]
    layer_index, component = _decode_layers(ids, [layer.shape[0] for layer in layers])
    dev = layers[0].device if layers else query_embeds.device
    return vals.to(dev), layer_index.to(dev), component.to(dev), names


@torch.no_grad()
def label_components(fm, vocabulary: list[str], aggregated_concept_db, k: int = 5, templates: list[str] | None = None,
                     batch_size: int | None = None, chunk_size: int | None = None):
    """For every component, its ``k`` best labels out of ``vocabulary``: ``(values (C, k) float32, ids (C, k) int64)`` for a
    ``(C, D)`` tensor, a dict of such pairs for a dict of layers, on the DB's device; ``ids`` index ``vocabulary``.

    The vocabulary is embedded ``chunk_size`` words at a time (default ``LABEL_CHUNK_WORDS``; ``batch_size`` is the text
    tower's batch, as in ``text_probing``), each chunk goes through one cosine GEMM per layer — the DB as rows, the chunk as
    columns — and is folded into the layers' top-k states.  Neither the ``V x C`` similarity matrix nor, for
    ``chunk_size < V``, all ``V x D`` embeddings are ever resident.

    Templates: each word's embedding is the mean over ITS OWN templated prompts minus the empty-template embedding.
    ``text_probing`` instead reproduces the reference's regrouping, which mixes the queries of one call and so depends on
    the whole list; that cannot survive chunking and is deliberately not reproduced here (for a single query the two
    agree).  With ``templates=None`` a word's embedding is exactly ``fm.encode_text(fm.tokenize([w]))``'s row.

    ``k``, the vocabulary, ``chunk_size`` and the DB's shape are checked before anything runs.  The text tower's width is
    not known until it has produced an embedding, so a ``D`` mismatch raises ``ValueError`` only after the first chunk has
    been embedded (and the DB has been moved to the device); nothing has been multiplied by then."""
    k = N.check_topk_k(k)
    if isinstance(vocabulary, str) or not isinstance(vocabulary, (list, tuple)) or len(vocabulary) == 0:
        raise ValueError("vocabulary must be a non-empty list of strings")
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    chunks = _embedded_chunks(fm, list(vocabulary), layers, templates, batch_size, chunk_size)
    dbs = [N._f32c(layer) for layer in layers]  # raises without a HIP device, before the text tower runs
    states = [None] * len(dbs)
    for start, _, embeds in chunks:
        for i, db in enumerate(dbs):
            states[i] = N.topk_probe(db, embeds, k, id_base=start, state=states[i])
    out = {name: (vals.to(layer.device), ids.to(layer.device)) for name, layer, (vals, ids) in zip(names, layers, states)}
    return out if is_dict else out[None]


# ------------------------------------------------------------------------------------------------
# describe, calibrated: softmax over the whole vocabulary next to the top-k (K17 + K25 on the same tiles)
# ------------------------------------------------------------------------------------------------
@dataclass
class LabelDistribution:
    """What ``label_distribution`` returns for one layer: ``label_components``' top-k next to
    ``softmax(logit_scale * cosine)`` taken over the WHOLE vocabulary.

    * ``values`` / ``ids`` ``(C, k)``: ``label_components``' result, bit for bit.
    * ``probs (C, k)`` float32: the probability of each returned label (0 in an empty slot, ``k > n_labels``).
    * ``log_z`` / ``entropy`` ``(C,)`` float64: the log partition sum of ``logit_scale * cosine`` and the entropy in nats.

    A component whose cosines hold a NaN has NaN everywhere; nothing filters it."""

    values: torch.Tensor
    ids: torch.Tensor
    probs: torch.Tensor
    log_z: torch.Tensor
    entropy: torch.Tensor
    n_labels: int
    logit_scale: float

    @property
    def effective_labels(self) -> torch.Tensor:
        """``exp(entropy)``: how many labels a component is really spread over, between 1 and ``n_labels``."""
        return self.entropy.exp()

    def confident(self, min_prob: float = 0.5) -> torch.Tensor:
        """``(C,)`` bool: the best label holds at least ``min_prob``; ``False`` where the distribution is NaN."""
        return self.probs[:, 0] >= min_prob


@torch.no_grad()
def probe_softmax(query_embeds: torch.Tensor, aggregated_concept_db, k: int, logit_scale: float = 100.0, chunk_rows: int | None = None):
    """``probe_topk(per="component")`` with the softmax over ALL queries: per component
    ``(values (C, k), ids (C, k), probs (C, k) float32, log_z (C,) float64, entropy (C,) float64)``, a dict of such tuples for a
    dict DB.  ``values`` / ``ids`` are ``probe_topk``'s; ``probs[c, i] = exp(logit_scale * values[c, i] - log_z[c])`` where ``log_z``
    is the log-sum-exp of ``logit_scale * cosine`` over every row of ``query_embeds``.  The ``(C, Q)`` matrix is never formed: K25
    folds each tile K17 reads into a four-double state per component."""
    k = N.check_topk_k(k)
    scale = N.check_logit_scale(logit_scale)
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    _check_width(query_embeds, layers)
    for layer in layers:  # the probe's own check, made here too because _probe_layers moves a layer to the device before it probes
        N._check_probe_args("probe_softmax", layer, query_embeds, chunk_rows=chunk_rows)

    def probe(ld, q):
        vals, ids, sm = N.softmax_probe(ld, q, k, scale, chunk_rows)
        return (vals, ids, *N.softmax_finish(sm, scale, vals))

    return _probe_layers(names, layers, is_dict, query_embeds, probe)


@torch.no_grad()
def label_distribution(fm, vocabulary: list[str], aggregated_concept_db, k: int = 5, logit_scale: float = 100.0,
                       templates: list[str] | None = None, batch_size: int | None = None, chunk_size: int | None = None):
    """``label_components`` plus how much each label means: a ``LabelDistribution`` (a dict of them for a dict of layers) with the
    same ``values`` / ``ids`` and, per component, ``softmax(logit_scale * cosine)`` over the whole vocabulary — the probability of
    the ``k`` returned labels, the log partition sum and the entropy.  Raw cosines sit on a large common offset and cannot be
    compared across components; ``probs[:, 0]`` and ``effective_labels`` can, and ``confident()`` says which components have a label
    worth printing.  ``logit_scale``: the CLIP family trains with about 100.

    Vocabulary, templates, ``batch_size``, ``chunk_size`` and what is checked before anything runs are ``label_components``'; the
    softmax statistics are folded (K25) from the very tiles its top-k reads, so there is one GEMM per tile and no ``V x C`` matrix.
    Chunking changes ``probs``, ``log_z`` and ``entropy`` only within the rounding bound of DESIGN.md §K25.

    For a ``Facets`` pass ``facets.aggregated()``, as with ``audit_concepts``.  An empty facet's row is all zeros, its cosine to
    every word is 0, so its distribution is uniform: ``probs = 1 / n_labels``, ``effective_labels = n_labels``."""
    k = N.check_topk_k(k)
    scale = N.check_logit_scale(logit_scale)
    if isinstance(vocabulary, str) or not isinstance(vocabulary, (list, tuple)) or len(vocabulary) == 0:
        raise ValueError("vocabulary must be a non-empty list of strings")
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    chunks = _embedded_chunks(fm, list(vocabulary), layers, templates, batch_size, chunk_size)
    dbs = [N._f32c(layer) for layer in layers]  # raises without a HIP device, before the text tower runs
    states = [None] * len(dbs)
    for start, _, embeds in chunks:
        for i, db in enumerate(dbs):
            states[i] = N.softmax_probe(db, embeds, k, scale, id_base=start, state=states[i])
    out = {}
    for name, layer, (vals, ids, sm) in zip(names, layers, states):
        tensors = (vals, ids, *N.softmax_finish(sm, scale, vals))
        out[name] = LabelDistribution(*(t.to(layer.device) for t in tensors), n_labels=len(vocabulary), logit_scale=scale)
    return out if is_dict else out[None]


# ------------------------------------------------------------------------------------------------
# describe, without the hubs: labels ranked by CSLS, not by the raw cosine (K6 + K17 twice for the densities, K29)
# ------------------------------------------------------------------------------------------------
@dataclass
class HubnessLabels:
    """What ``label_components_csls`` / ``probe_csls`` return for one layer: per component its ``k`` best labels under the CSLS
    score ``2 cos(x_i, w_j) - r_i - q_j`` (Conneau et al. 2018), which discounts a cosine by how crowded both ends' neighbourhoods are.

    * ``values (C, k)`` float32: the scores, best first (K17's order on the score: NaN first, larger first, ties by the smaller
      id); ``-inf`` in an unused slot (``k`` beyond the vocabulary).
    * ``ids (C, k)`` int64: index the vocabulary; ``-1`` unused.
    * ``component_density (C,)`` float32: ``r``, the mean of the component's ``neighbours`` largest cosines over the vocabulary.
    * ``label_density (V,)`` float32: ``q``, the mean of the word's ``neighbours`` largest cosines over THIS layer's components: how
      much of a hub the word is here.
    * ``neighbours``: the neighbourhood size; with fewer candidates on a side the density is the mean over those present."""

    values: torch.Tensor
    ids: torch.Tensor
    component_density: torch.Tensor
    label_density: torch.Tensor
    neighbours: int

    @property
    def cosine(self) -> torch.Tensor:
        """``(C, k)`` float32: the cosine of each returned pair, recovered as ``float32((float64(score) + r_i + q_id) / 2)`` — within
        1.5e-7 of the cosine the score was taken from; NaN in an unused slot."""
        present = self.ids >= 0
        q = self.label_density.to(torch.float64)[self.ids.clamp(min=0)] if self.label_density.numel() else 0.0
        cos = (self.values.to(torch.float64) + self.component_density.to(torch.float64)[:, None] + q) / 2
        return torch.where(present, cos, float("nan")).to(torch.float32)

    def hubs(self, n: int = 20):
        """``(values, ids)`` of the ``n`` words of largest ``label_density``, largest first (a NaN density before every number, equal
        densities by the smaller id): the hubs themselves, worth printing once per layer."""
        n = operator.index(n)
        if n < 0:
            raise ValueError(f"n = {n} must not be negative")
        vals, ids = torch.sort(self.label_density, descending=True, stable=True)
        return vals[:n], ids[:n]


def _check_csls_args(k, neighbours, chunk_rows=None):
    k, neighbours = N.check_topk_k(k), N.check_neighbours(neighbours)
    if chunk_rows is not None and chunk_rows < 1:
        raise ValueError(f"chunk_rows = {chunk_rows} must be at least 1")
    return k, neighbours


def _csls_layers(names, layers, is_dict, vocab_embeds: torch.Tensor, k: int, neighbours: int, chunk_rows):
    """``N.csls_probe`` per layer against ONE resident vocabulary (moved only when a layer lives on another device); each layer has
    its own label densities; results on the device each layer came from."""
    out, w = {}, None
    for name, layer in zip(names, layers):
        db = N._f32c(layer)
        if w is None or w.device != db.device:
            w = N._f32c(vocab_embeds, db.device)
        vals, ids, r, q = N.csls_probe(db, w, k, neighbours, chunk_rows)
        out[name] = HubnessLabels(*(t.to(layer.device) for t in (vals, ids, r, q)), neighbours=neighbours)
    return out if is_dict else out[None]


@torch.no_grad()
def probe_csls(vocab_embeds: torch.Tensor, aggregated_concept_db, k: int = 5, neighbours: int = 10, chunk_rows: int | None = None):
    """``probe_topk(per="component")`` ranked by CSLS instead of the raw cosine, for callers who bring their own vectors: a
    ``HubnessLabels`` for a ``(C, D)`` tensor, a dict of them for a dict of layers.

    ``csls(i, j) = 2 cos(x_i, w_j) - r_i - q_j`` with ``r_i`` the mean of component ``i``'s ``neighbours`` (1 to 1 024) largest cosines
    over ``vocab_embeds (V, D)`` and ``q_j`` the mean of word ``j``'s ``neighbours`` largest cosines over the layer's components.  A
    word that is close to every component (a hub: "photo", a template's residue) has a large ``q`` and loses its lead to the word
    that is close to this component only.  Three passes of the cosine GEMM (K6) per layer, none of which forms the ``(C, V)``
    matrix: K17 over components x words gives ``r``, K17 over words x components gives ``q``, and K29 folds the tiles of the third
    ranking them by the score, computed in registers.  ``V x D x 4`` bytes of ``vocab_embeds`` stay on the device throughout.

    A NaN cosine or density makes the score NaN, and a NaN ranks first, as in ``label_components``.  ``chunk_rows``: as in
    ``probe_topk``.  Arguments are checked before a device is touched."""
    k, neighbours = _check_csls_args(k, neighbours, chunk_rows)
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    if not isinstance(vocab_embeds, torch.Tensor):
        raise ValueError(f"vocab_embeds must be a (V, D) tensor, got {type(vocab_embeds).__name__}")
    _check_width(vocab_embeds, layers)
    if vocab_embeds.shape[0] == 0:
        raise ValueError("vocab_embeds holds no rows")
    return _csls_layers(names, layers, is_dict, vocab_embeds, k, neighbours, chunk_rows)


@torch.no_grad()
def label_components_csls(fm, vocabulary: list[str], aggregated_concept_db, k: int = 5, neighbours: int = 10,
                          templates: list[str] | None = None, batch_size: int | None = None, chunk_size: int | None = None,
                          chunk_rows: int | None = None):
    """``label_components`` with the hubs discounted: for every component its ``k`` best labels out of ``vocabulary`` under the CSLS
    score (``probe_csls`` states it), as a ``HubnessLabels`` for a ``(C, D)`` tensor, a dict of them for a dict of layers (for a
    ``Facets``, pass ``facets.aggregated()``), on the DB's device.  Raw cosines sit on a large common offset, and the few words that
    lie near it head the top-5 of most components; here they are scored down by their own density (``hl.hubs()`` lists them) and the
    word that tells a component apart comes first.  Each layer is independent: ``label_density`` is taken over that layer's components.

    The vocabulary is embedded once, ``chunk_size`` words at a time exactly as ``label_components`` embeds it (templates included),
    into ONE resident ``(V, D)`` fp32 device tensor: both densities need the whole vocabulary before the scoring pass can start, so
    ``V x D x 4`` bytes must fit on the device (410 MB for 100 000 words of width 1 024) — unlike ``label_components``, which never
    holds more than a chunk.  A NaN cosine or density makes the score NaN, and a NaN ranks first, as in ``label_components``.
    ``k``, ``neighbours``, ``chunk_rows``, the vocabulary, ``chunk_size`` and the DB's shape are checked before the text tower or a device
    is touched; a ``D`` mismatch can only raise once the first chunk is embedded."""
    k, neighbours = _check_csls_args(k, neighbours, chunk_rows)
    if isinstance(vocabulary, str) or not isinstance(vocabulary, (list, tuple)) or len(vocabulary) == 0:
        raise ValueError("vocabulary must be a non-empty list of strings")
    vocabulary = list(vocabulary)
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    w = _embed_vocabulary(fm, vocabulary, layers, templates, batch_size, chunk_size)
    return _csls_layers(names, layers, is_dict, w, k, neighbours, chunk_rows)


# ------------------------------------------------------------------------------------------------
# describe, evaluated: where an expected label stands among all V words (K26 on the tiles K17 reads)
# ------------------------------------------------------------------------------------------------
@dataclass
class LabelRanks:
    """What ``label_rank`` / ``probe_rank`` return for one layer: per component and target slot, the position the target holds
    when the component's cosines to all ``n_labels`` words are sorted in ``label_components``' order.

    * ``rank (C, T)`` int64: 0 = the target is the top label; -1 in an unused slot.
    * ``value (C, T)`` float32: the target's cosine; NaN in an unused slot.
    * ``targets (C, T)`` int64: the vocabulary indices asked for, -1 = unused.
    * ``prob (C, T)`` float32 = ``exp(logit_scale * value - log_z)`` and ``log_z (C,)`` float64, the log partition sum over the
      whole vocabulary (``label_distribution``'s); both ``None`` without a ``logit_scale``.

    A target is *valid* when it is used and its cosine is not NaN.  ``rank`` follows the order as it is — a NaN target ranks
    first, as it would in ``label_components`` — while ``best``, ``hit`` and the metrics leave NaN targets out."""

    rank: torch.Tensor
    value: torch.Tensor
    targets: torch.Tensor
    prob: torch.Tensor | None
    log_z: torch.Tensor | None
    n_labels: int
    logit_scale: float | None = None

    def _valid(self) -> torch.Tensor:
        return (self.targets >= 0) & ~self.value.isnan()

    def best(self) -> torch.Tensor:
        """``(C,)`` int64: the smallest rank over the component's valid targets (synonyms), -1 without one."""
        valid = self._valid()
        best = self.rank.masked_fill(~valid, torch.iinfo(torch.int64).max).amin(dim=1)
        return best.masked_fill(~valid.any(dim=1), -1)

    def hit(self, k: int) -> torch.Tensor:
        """``(C,)`` bool: a valid target is among the component's ``k`` best labels."""
        best = self.best()
        return (best >= 0) & (best < k)

    @property
    def n_evaluated(self) -> int:
        """The number of components with at least one valid target: what the metrics average over."""
        return int(self._valid().any(dim=1).sum())

    def topk_accuracy(self, k: int) -> float:
        """The share of evaluated components with ``hit(k)``; NaN when none is evaluated."""
        n = self.n_evaluated
        return float(self.hit(k).sum()) / n if n else float("nan")

    def mrr(self) -> float:
        """Mean reciprocal rank ``1 / (best() + 1)`` over the evaluated components; NaN when none is evaluated."""
        best = self.best()
        best = best[best >= 0]
        return float((1.0 / (best.double() + 1.0)).mean()) if best.numel() else float("nan")


def _rank_layers(aggregated_concept_db, targets):
    """``(names, layers, is_dict, per-layer targets)`` for the layers ``targets`` names: all of a tensor DB, a subset of a dict DB."""
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    if not is_dict:
        if isinstance(targets, Mapping):
            raise ValueError("targets is a dict but the concept DB is a single tensor")
        return names, layers, is_dict, [targets]
    if not isinstance(targets, Mapping):
        raise ValueError("for a dict of layers, targets must be a dict over (a subset of) its layer names")
    unknown = [name for name in targets if name not in aggregated_concept_db]
    if unknown:
        raise ValueError(f"targets names unknown layers {unknown}; the concept DB has {names}")
    keep = [i for i, name in enumerate(names) if name in targets]
    return [names[i] for i in keep], [layers[i] for i in keep], is_dict, [targets[names[i]] for i in keep]


def _resolve_targets(targets, n_components: int, n_labels: int, vocabulary=None, index=None) -> torch.Tensor:
    """One layer's targets as ``N.check_rank_targets``' ``(C, T)`` tensor; words are looked up in ``vocabulary`` (first occurrence,
    through ``index``, a dict the caller keeps across layers)."""
    if hasattr(targets, "tolist"):  # a tensor or an array holds indices only
        return N.check_rank_targets(targets, n_components, n_labels)
    if isinstance(targets, (str, bytes)) or not isinstance(targets, (list, tuple)):
        raise ValueError(f"targets must hold one entry per component, got {type(targets).__name__}")

    def lookup(item):
        if not isinstance(item, str):
            return item
        if vocabulary is None:
            raise ValueError(f"target {item!r} is a word, but there is no vocabulary to look it up in: pass indices")
        if not index:
            for i, word in enumerate(vocabulary):
                index.setdefault(word, i)
        if item not in index:
            raise ValueError(f"target word {item!r} is not in the vocabulary")
        return index[item]

    resolved = [[lookup(i) for i in entry] if isinstance(entry, (list, tuple)) else lookup(entry) for entry in targets]
    return N.check_rank_targets(resolved, n_components, n_labels)


def _rank_result(layer, targets, key_vals, counts, sm, scale, n_labels: int) -> LabelRanks:
    used = targets >= 0
    rank = counts.masked_fill(~used, -1)
    prob = log_z = None
    if sm is not None:
        _, log_z, _ = N.softmax_finish(sm, scale)
        prob = (scale * key_vals.double() - log_z[:, None]).exp().float()
    dev = layer.device
    return LabelRanks(rank.to(dev), key_vals.to(dev), targets.to(dev), None if prob is None else prob.to(dev),
                      None if log_z is None else log_z.to(dev), n_labels, scale)


@torch.no_grad()
def probe_rank(query_embeds: torch.Tensor, aggregated_concept_db, targets, chunk_rows: int | None = None,
               logit_scale: float | None = None):
    """For every component, where expected queries stand among ALL rows of ``query_embeds (Q, D)``: a ``LabelRanks`` (a dict of
    them for a dict DB), for callers who bring their own vectors.  ``targets``: per component a row index of ``query_embeds``, a
    list of up to 16 of them, or ``None``; for a dict DB a dict over a subset of its layers, and only those are ranked.

    ``rank[c, t]`` is the number of queries that ``probe_topk(per="component")`` would list before the target: given the targets'
    cosines and the tiles' cosines it is exact, and ``rank[c, t] < k`` can disagree with membership in ``probe_topk``'s ids, or with
    the float64 rank, only by candidates whose cosine lies within the cosine GEMM's rounding of the target's.  The ``(C, Q)`` matrix
    is never formed: the targets' cosines are taken through the same GEMM first, then K26 counts, per tile K17 would read, the
    candidates that order before them.  With ``logit_scale``, K25 folds the same tiles and ``prob`` / ``log_z`` are filled."""
    scale = None if logit_scale is None else N.check_logit_scale(logit_scale)
    if chunk_rows is not None and chunk_rows < 1:
        raise ValueError(f"chunk_rows = {chunk_rows} must be at least 1")
    names, layers, is_dict, per_layer = _rank_layers(aggregated_concept_db, targets)
    _check_width(query_embeds, layers)
    n = query_embeds.shape[0]
    resolved = [_resolve_targets(t, layer.shape[0], n) for t, layer in zip(per_layer, layers)]
    out, q = {}, None
    for name, layer, tg in zip(names, layers, resolved):
        db = N._f32c(layer)
        q = N._f32c(query_embeds, db.device) if q is None or q.device != db.device else q
        key_vals = N.rank_keys(db, q, tg, chunk_rows)  # the targets are still on the host: its checks cost no readback
        tg = tg.to(db.device)
        sm = N.softmax_new(db.shape[0], db.device) if scale is not None else None
        counts = N.rank_probe(db, q, key_vals, tg, chunk_rows, softmax=None if sm is None else (sm, scale))
        out[name] = _rank_result(layer, tg, key_vals, counts, sm, scale, n)
    return out if is_dict else out[None]


@torch.no_grad()
def label_rank(fm, vocabulary: list[str], aggregated_concept_db, targets, templates: list[str] | None = None,
               batch_size: int | None = None, chunk_size: int | None = None, logit_scale: float | None = None):
    """For labels you expect, where they stand among all of ``vocabulary``: a ``LabelRanks`` (a dict of them for a dict of layers)
    whose ``rank[c, t]`` is the 0-based position of target ``t`` in the list ``label_components`` would return for component ``c``
    with ``k = len(vocabulary)`` — the number a labelling is evaluated with (``hit``, ``topk_accuracy``, ``mrr``).

    ``targets``: per component a vocabulary index, a word (looked up in ``vocabulary``, first occurrence; an absent word is a
    ``ValueError``), a list of up to 16 of either (synonyms), or ``None``.  For a dict DB a dict over a subset of its layers: only
    those layers are ranked and returned.

    The unique target words are embedded first, with the same templates as the vocabulary, and their cosines taken through the
    cosine GEMM; then the vocabulary is streamed exactly as ``label_components`` streams it and K26 counts, per tile, the words
    that order before each target.  Neither the ``V x C`` matrix nor, for ``chunk_size < V``, all embeddings are ever resident; the
    target words are embedded twice.  Given the targets' cosines and the tiles' cosines the rank is exact; it can differ from
    the float64 rank, and ``rank < k`` from membership in ``label_components``' ids, only by words whose cosine lies within the
    cosine GEMM's rounding of the target's.  With ``logit_scale``, ``prob`` / ``log_z`` are ``label_distribution``'s softmax over the
    whole vocabulary (K25 on the same tiles).  Arguments are checked before anything runs, as in ``label_components``."""
    scale = None if logit_scale is None else N.check_logit_scale(logit_scale)
    if isinstance(vocabulary, str) or not isinstance(vocabulary, (list, tuple)) or len(vocabulary) == 0:
        raise ValueError("vocabulary must be a non-empty list of strings")
    vocabulary = list(vocabulary)
    names, layers, is_dict, per_layer = _rank_layers(aggregated_concept_db, targets)
    index = {}
    resolved = [_resolve_targets(t, layer.shape[0], len(vocabulary), vocabulary, index) for t, layer in zip(per_layer, layers)]
    chunks = _embedded_chunks(fm, vocabulary, layers, templates, batch_size, chunk_size)
    dbs = [N._f32c(layer) for layer in layers]  # raises without a HIP device, before the text tower runs
    # the targets' cosines: the unique target words of all layers, embedded once
    uniq = torch.unique(torch.cat([t[t >= 0] for t in resolved])) if resolved else torch.empty(0, dtype=torch.int64)
    key_ids = [t.to(db.device) for t, db in zip(resolved, dbs)]
    if uniq.numel():
        embeds = _embed_words(fm, [vocabulary[i] for i in uniq.tolist()], templates, batch_size)
        _check_width(embeds, layers)
        key_vals = [N.rank_keys(db, embeds, torch.searchsorted(uniq, t.clamp(min=0)).masked_fill(t < 0, -1))
                    for db, t in zip(dbs, resolved)]
        del embeds
    else:
        key_vals = [torch.full(t.shape, float("nan"), dtype=torch.float32, device=t.device) for t in key_ids]
    counts = [None] * len(dbs)
    sms = [N.softmax_new(db.shape[0], db.device) if scale is not None else None for db in dbs]
    for start, _, embeds in chunks:
        for i, db in enumerate(dbs):
            counts[i] = N.rank_probe(db, embeds, key_vals[i], key_ids[i], id_base=start, state=counts[i],
                                     softmax=None if sms[i] is None else (sms[i], scale))
    out = {name: _rank_result(layer, key_ids[i], key_vals[i], counts[i], sms[i], scale, len(vocabulary))
           for i, (name, layer) in enumerate(zip(names, layers))}
    return out if is_dict else out[None]


# ------------------------------------------------------------------------------------------------
# describe, jointly: which few words TOGETHER span a component (matching pursuit: K6 + K17 per pass, K28 between)
# ------------------------------------------------------------------------------------------------
@dataclass
class Decomposition:
    """What ``decompose_components`` / ``probe_decompose`` return for one layer: per component a sparse sum of words,
    ``x / |x| = sum_t coefs[t] * w[ids[t]] / |w[ids[t]]| + residual``, found greedily (orthogonal matching pursuit) with ``s`` terms
    at most.

    * ``ids (C, s)`` int64: the vocabulary index of term ``t``, in the order chosen; -1 in an unused slot.
    * ``coefs (C, s)`` float64: the least-squares weights of the unit-norm word vectors for the unit-norm component, solved over
      ALL chosen words (so they are the weights of the final set, not those at the moment of choice); 0.0 unused.
    * ``correlation (C, s)`` float32: the cosine between the residual and the word at the moment it was chosen; NaN unused.
    * ``explained (C, s)`` float64: ``1 - |residual|^2`` after ``t + 1`` terms, cumulative and non-decreasing; an unused slot repeats
      the last value (0.0 for a component without any term).
    * ``n_terms (C,)`` int32: terms used.  A component stops early when no unchosen word has a cosine above ``min_correlation``, when
      the best one depends linearly on the chosen ones (a duplicate vocabulary entry), or when ``|residual|^2 <= 1e-8``.
    * ``residual (C, D)`` float32: what the chosen words do not span, in units of the normalised component.

    A component that is a zero row or has a non-finite coordinate has ``n_terms`` 0, ``explained`` and ``residual`` NaN."""

    ids: torch.Tensor
    coefs: torch.Tensor
    correlation: torch.Tensor
    explained: torch.Tensor
    n_terms: torch.Tensor
    residual: torch.Tensor

    def terms(self, c: int, vocabulary) -> list:
        """``[(word, coef, explained)]`` of component ``c``, in the order the words were chosen."""
        n = int(self.n_terms[c])
        ids, coefs, explained = self.ids[c, :n].tolist(), self.coefs[c, :n].tolist(), self.explained[c, :n].tolist()
        return [(vocabulary[i], a, e) for i, a, e in zip(ids, coefs, explained)]


def _check_decompose_args(n_terms, min_correlation, chunk_rows=None):
    n_terms = N.check_omp_terms(n_terms)
    min_correlation = N.check_min_correlation(min_correlation)
    if chunk_rows is not None and chunk_rows < 1:
        raise ValueError(f"chunk_rows = {chunk_rows} must be at least 1")
    return n_terms, min_correlation


def _decompose_layers(names, layers, is_dict, vocab_embeds: torch.Tensor, n_terms: int, min_correlation: float, chunk_rows):
    """``N.decompose_probe`` per layer against ONE resident vocabulary (moved only when a layer lives on another device, checked
    finite once per device); results on the device each layer came from."""
    out, w = {}, None
    for name, layer in zip(names, layers):
        db = N._f32c(layer)
        if w is None or w.device != db.device:
            w = N._f32c(vocab_embeds, db.device)
            if not bool(torch.isfinite(w).all()):
                raise ValueError("the vocabulary embeddings hold a NaN or an infinite value")
        st = N.decompose_probe(db, w, n_terms, min_correlation, chunk_rows)
        dev = layer.device
        out[name] = Decomposition(st.ids.to(dev), st.coefs.to(dev), st.corr.to(dev), st.explained.to(dev), st.n_terms.to(dev),
                                  st.last.to(dev))
    return out if is_dict else out[None]


@torch.no_grad()
def probe_decompose(vocab_embeds: torch.Tensor, aggregated_concept_db, n_terms: int = 4, min_correlation: float = 0.0,
                    chunk_rows: int | None = None):
    """Decompose every component of a concept DB (a ``(C, D)`` tensor or a dict of layers) into a sparse sum of the rows of
    ``vocab_embeds (V, D)``, for callers who bring their own vectors: a ``Decomposition`` (a dict of them for a dict DB).

    Greedy orthogonal matching pursuit.  With ``r_0 = x / |x|`` and nothing chosen, step ``t`` of ``n_terms`` (1 to 16): the cosine
    GEMM (K6) and the streaming top-k (K17, ``k = t + 1``) give every residual's best words without the ``(C, V)`` matrix; one kernel
    (K28) takes per component the best word not chosen yet, stops the component if its cosine is NaN or ``<= min_correlation`` (finite,
    in ``[0, 1)``) or if the word depends linearly on the chosen ones, and otherwise solves the least squares over all chosen words in
    float64 and writes the new residual, recomputed from ``x``.  Cosines are signed: a word is chosen for pointing along the residual,
    not against it.  ``vocab_embeds`` must be finite (``ValueError``); ``V x D x 4`` bytes of it stay on the device throughout.
    ``chunk_rows``: as in ``probe_topk``.  Arguments are checked before a device is touched."""
    n_terms, min_correlation = _check_decompose_args(n_terms, min_correlation, chunk_rows)
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    if not isinstance(vocab_embeds, torch.Tensor):
        raise ValueError(f"vocab_embeds must be a (V, D) tensor, got {type(vocab_embeds).__name__}")
    _check_width(vocab_embeds, layers)
    if vocab_embeds.shape[0] == 0:
        raise ValueError("vocab_embeds holds no rows")
    return _decompose_layers(names, layers, is_dict, vocab_embeds, n_terms, min_correlation, chunk_rows)


@torch.no_grad()
def decompose_components(fm, vocabulary: list[str], aggregated_concept_db, n_terms: int = 4, templates: list[str] | None = None,
                         batch_size: int | None = None, chunk_size: int | None = None, min_correlation: float = 0.0,
                         chunk_rows: int | None = None):
    """For every component, the few words of ``vocabulary`` that TOGETHER span its embedding, with weights and the share left
    unexplained: a ``Decomposition`` for a ``(C, D)`` tensor, a dict of them for a dict of layers (for a ``Facets``, pass
    ``facets.aggregated()``), on the DB's device.  Where ``label_components`` scores every word on its own — so the five best labels
    of a component with two meanings are five synonyms of the dominant one — the pursuit removes what the chosen words explain
    before it looks for the next (``probe_decompose`` states the algorithm).

    The vocabulary is embedded once, ``chunk_size`` words at a time exactly as ``label_components`` embeds it (templates included),
    into ONE resident ``(V, D)`` fp32 device tensor: the pursuit revisits the whole vocabulary ``n_terms`` times and re-reads the rows
    it chose, so ``V x D x 4`` bytes must fit on the device (410 MB for 100 000 words of width 1 024) — unlike ``label_components``,
    which never holds more than a chunk.  ``n_terms``, ``min_correlation``, ``chunk_rows``, the vocabulary, ``chunk_size`` and the DB's
    shape are checked before the text tower or a device is touched; a ``D`` mismatch can only raise once the first chunk is embedded."""
    n_terms, min_correlation = _check_decompose_args(n_terms, min_correlation, chunk_rows)
    if isinstance(vocabulary, str) or not isinstance(vocabulary, (list, tuple)) or len(vocabulary) == 0:
        raise ValueError("vocabulary must be a non-empty list of strings")
    vocabulary = list(vocabulary)
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    w = _embed_vocabulary(fm, vocabulary, layers, templates, batch_size, chunk_size)
    return _decompose_layers(names, layers, is_dict, w, n_terms, min_correlation, chunk_rows)


@torch.no_grad()
def search_components(fm, query, aggregated_concept_db, k: int = 10, templates: list[str] | None = None,
                      batch_size: int | None = None):
    """The ``k`` components that best match each text query across ALL layers: ``(values (Q, k), layer_index (Q, k),
    component (Q, k), layer_names)`` (see ``probe_topk(per="query")``).  Templates are applied per query, as in
    ``label_components``; as there, a ``D`` mismatch can only raise once the text tower has embedded the queries."""
    k = N.check_topk_k(k)
    queries = list(query) if isinstance(query, (list, tuple)) else [query]
    if not queries:
        raise ValueError("search_components needs at least one query")
    _, layers, _ = _db_layers(aggregated_concept_db)
    for layer in layers:
        N._f32c(layer)  # raises without a HIP device, before the text tower runs
    return probe_topk(_embed_words(fm, queries, templates, batch_size), aggregated_concept_db, k, per="query")


@torch.no_grad()
def search_components_image(fm, query, aggregated_concept_db, k: int = 10):
    """``search_components`` for an image query (several images are averaged, as in ``image_probing``): one result row.
    ``k`` and the DB's shape are checked first; the image tower's width is only known from its output, so a ``D`` mismatch
    raises ``ValueError`` after the tower has run and before any similarity is computed."""
    k = N.check_topk_k(k)
    _db_layers(aggregated_concept_db)
    return probe_topk(_embed_image_probe(fm, query), aggregated_concept_db, k, per="query")


# ------------------------------------------------------------------------------------------------
# facets: describe / search the meanings of a polysemantic component (K9's labels + K21)
# ------------------------------------------------------------------------------------------------
def _facet_layers(facets):
    """``(names, [Facets], is_dict)`` of a ``Facets`` or a dict of them."""
    is_dict = not isinstance(facets, Facets)
    if is_dict and not isinstance(facets, dict):
        raise ValueError(f"facets must be a Facets or a dict of them, got {type(facets).__name__}")
    names = list(facets) if is_dict else [None]
    layers = [facets[n] for n in names] if is_dict else [facets]
    for name, f in zip(names, layers):
        if not isinstance(f, Facets) or f.centers.ndim != 3 or tuple(f.counts.shape) != tuple(f.centers.shape[:2]):
            raise ValueError(f"layer {name!r} is not a Facets with centers (C, kc, D) and counts (C, kc)")
    return names, layers, is_dict


@torch.no_grad()
def label_facets(fm, vocabulary: list[str], facets, k: int = 5, templates: list[str] | None = None, batch_size: int | None = None,
                 chunk_size: int | None = None):
    """For every facet of every component, its ``k`` best labels out of ``vocabulary``: ``(values (C, kc, k) float32, ids
    (C, kc, k) int64)`` for a ``Facets``, a dict of such pairs for a dict of them.  It is ``label_components`` on
    ``facets.aggregated()``, reshaped; the slots of an empty facet (``count == 0``: its centre is all zeros, its cosines mean
    nothing) hold ``-inf`` / ``-1``, the unused-slot convention of ``probe_topk``."""
    names, layers, is_dict = _facet_layers(facets)
    db = {i: f.aggregated() for i, f in enumerate(layers)}
    labelled = label_components(fm, vocabulary, db, k, templates, batch_size, chunk_size)  # checks its arguments first
    out = {}
    for i, (name, f) in enumerate(zip(names, layers)):
        vals, ids = labelled[i]
        C, kc = f.counts.shape
        vals, ids = vals.reshape(C, kc, -1), ids.reshape(C, kc, -1)
        empty = (f.counts == 0).to(vals.device)[..., None]
        out[name] = (vals.masked_fill(empty, float("-inf")), ids.masked_fill(empty, -1))
    return out if is_dict else out[None]


@torch.no_grad()
def search_facets(fm, query, facets, k: int = 10, templates: list[str] | None = None):
    """The ``k`` facets that best match each text query across ALL layers: ``(values (Q, k), layer_index (Q, k), component
    (Q, k), facet (Q, k), layer_names)``.  It is ``search_components`` over the layers' aggregated facet DBs with the row
    decoded as ``(row // kc, row % kc)``; empty facets are dropped before probing, so they never appear.  Unused slots hold
    ``-inf`` / ``-1``."""
    k = N.check_topk_k(k)
    names, layers, _ = _facet_layers(facets)
    keeps = [(f.counts.reshape(-1) > 0).nonzero()[:, 0] for f in layers]  # rows of aggregated() that hold a facet
    db = {i: f.aggregated()[keep.to(f.centers.device)] for i, (f, keep) in enumerate(zip(layers, keeps))}
    vals, layer_index, row, _ = search_components(fm, query, db, k, templates)
    dev = row.device
    sizes = torch.tensor([keep.numel() for keep in keeps], dtype=torch.int64, device=dev)
    kcs = torch.tensor([f.n_clusters for f in layers], dtype=torch.int64, device=dev)
    kept = torch.cat([keep.to(dev) for keep in keeps]) if keeps else torch.zeros(0, dtype=torch.int64, device=dev)
    empty = row < 0
    layer = layer_index.clamp(min=0)
    if kept.numel():
        original = kept[((sizes.cumsum(0) - sizes)[layer] + row).masked_fill(empty, 0)]
    else:
        original = torch.zeros_like(row)
    kc = kcs[layer] if kcs.numel() else torch.ones_like(row)
    component = torch.div(original, kc, rounding_mode="floor").masked_fill(empty, -1)
    facet = (original % kc).masked_fill(empty, -1)
    return vals, layer_index, component, facet, names


# ------------------------------------------------------------------------------------------------
# compare: two concept DBs against each other, both directions from one cosine pass (K6 tiles + K20)
# ------------------------------------------------------------------------------------------------
@dataclass
class ConceptDBComparison:
    """What ``compare_concept_dbs`` returns.  Every tensor lives on DB A's device.

    * ``layers_a`` / ``layers_b``: the layer names (``[None]`` for a tensor DB); ``sizes_a`` / ``sizes_b``: their component counts.
    * ``pairs[(i, j)]`` = ``(vals_a (Ca,), ids_a (Ca,), vals_b (Cb,), ids_b (Cb,))`` for A's layer ``i`` and B's layer ``j``: every
      A component's best cosine in that B layer and the B component that has it, and the reverse.  ``pair(name_a, name_b)`` reads
      it by name.
    * ``best_ab[i]`` = ``(values (Ca,), ids (Ca,))``: every component of A's layer ``i`` against ALL of B, ``ids`` being B's global
      component ids ``offset[layer] + component``; ``best_ba[j]`` the reverse.  ``best_in_b`` / ``best_in_a`` decode them.

    A NaN cosine (a NaN in an embedding) ranks before every number, so it becomes the best match of its row and column and
    turns the means it enters into NaN; nothing filters it."""

    layers_a: list
    layers_b: list
    sizes_a: list[int]
    sizes_b: list[int]
    pairs: dict
    best_ab: list
    best_ba: list

    def pair(self, name_a=None, name_b=None):
        """``(vals_a, ids_a, vals_b, ids_b)`` of one layer pair."""
        return self.pairs[(self.layers_a.index(name_a), self.layers_b.index(name_b))]

    def _layer_similarity(self, side: int) -> torch.Tensor:
        La, Lb = len(self.layers_a), len(self.layers_b)
        rows = [[self.pairs[(i, j)][side].mean() for j in range(Lb)] for i in range(La)]
        if side:  # the pair's B -> A half: (Lb, La)
            rows = [[rows[i][j] for i in range(La)] for j in range(Lb)]
        return torch.stack([torch.stack(r) for r in rows])

    @property
    def layer_similarity_ab(self) -> torch.Tensor:
        """``(La, Lb)`` float32: the mean over an A layer's components of their best cosine in a B layer."""
        return self._layer_similarity(0)

    @property
    def layer_similarity_ba(self) -> torch.Tensor:
        """``(Lb, La)`` float32: the mean over a B layer's components of their best cosine in an A layer."""
        return self._layer_similarity(2)

    @property
    def set_similarity_ab(self) -> float:
        """``mean_i max_j cos(a_i, b_j)`` over ALL of A's components against all of B (fp32 mean on the device)."""
        return float(torch.cat([v for v, _ in self.best_ab]).mean())

    @property
    def set_similarity_ba(self) -> float:
        return float(torch.cat([v for v, _ in self.best_ba]).mean())

    @property
    def best_in_b(self) -> dict:
        """``{name_a: (values (Ca,), layer_index (Ca,), component (Ca,))}``: the best match across all of B's layers (ties between
        layers go to the earlier layer, then to the smaller component)."""
        return {name: (v,) + _decode_layers(g, self.sizes_b) for name, (v, g) in zip(self.layers_a, self.best_ab)}

    @property
    def best_in_a(self) -> dict:
        return {name: (v,) + _decode_layers(g, self.sizes_a) for name, (v, g) in zip(self.layers_b, self.best_ba)}

    def mutual(self) -> dict:
        """``{name_a: bool (Ca,)}``: component ``a``'s best match in B has ``a`` as ITS best match in A (mutual nearest neighbours)."""
        to_b = torch.cat([g for _, g in self.best_ab])  # per global A id: its best global B id
        to_a = torch.cat([g for _, g in self.best_ba])
        back = to_a[to_b.clamp(min=0)]
        mask = (to_b >= 0) & (back == torch.arange(to_b.numel(), device=to_b.device))
        return dict(zip(self.layers_a, mask.split(self.sizes_a)))


def _merge_best(per_layer, offsets):
    """The best of several layers' ``k = 1`` results ``[(vals (C,), ids (C,)), ...]`` under K17's order, as ``(values (C,), global
    ids (C,))`` with ``global id = offsets[layer] + id``."""
    C, dev = per_layer[0][0].shape[0], per_layer[0][0].device
    vals, ids = N.topk_new(C, 1, dev)
    other_v = torch.stack([v for v, _ in per_layer], dim=1)
    other_i = torch.stack([torch.where(i < 0, i, i + off) for (_, i), off in zip(per_layer, offsets)], dim=1)
    N.topk_merge_states(vals, ids, other_v, other_i)
    return vals[:, 0], ids[:, 0]


@torch.no_grad()
def compare_concept_dbs(aggregated_concept_db_a, aggregated_concept_db_b, chunk_rows: int | None = None) -> ConceptDBComparison:
    """Compare two aggregated concept DBs (``(C, D)`` tensors or dicts of layers) embedded by the same foundation model: which
    components of A have a counterpart in B and the reverse, and how similar each layer of A is to each layer of B — the
    directed set similarity ``S(A -> B) = mean_i max_j cos(a_i, b_j)`` per layer pair and overall, in both directions.

    One ``_native.mutual_probe`` per layer pair: the cosine GEMM writes one tile at a time and K20 takes the row maxima (A -> B)
    and the column maxima (B -> A) out of the same read, so each product is computed once and no ``(Ca, Cb)`` matrix exists.
    The best match across layers is a merge of the per-pair results under the order of ``probe_topk``.  Always
    ``normalize(a) @ normalize(b).T``.  Shapes are checked before a device is touched; see ``ConceptDBComparison``."""
    names_a, layers_a, _ = _db_layers(aggregated_concept_db_a)
    names_b, layers_b, _ = _db_layers(aggregated_concept_db_b)
    for what, layers in (("A", layers_a), ("B", layers_b)):
        if not layers or any(layer.shape[0] == 0 for layer in layers):
            raise ValueError(f"concept DB {what} is empty (no layers, or a layer without components)")
    _check_width(layers_b[0], layers_a)
    da = [N._f32c(layer) for layer in layers_a]
    db = [N._f32c(layer, da[0].device) for layer in layers_b]
    out_dev = layers_a[0].device
    sizes_a, sizes_b = [t.shape[0] for t in da], [t.shape[0] for t in db]
    pairs = {(i, j): N.mutual_probe(a, b, chunk_rows) for i, a in enumerate(da) for j, b in enumerate(db)}
    off_a = [sum(sizes_a[:i]) for i in range(len(da))]
    off_b = [sum(sizes_b[:j]) for j in range(len(db))]
    best_ab = [_merge_best([pairs[(i, j)][0] for j in range(len(db))], off_b) for i in range(len(da))]
    best_ba = [_merge_best([pairs[(i, j)][1] for i in range(len(da))], off_a) for j in range(len(db))]
    to = lambda ts: tuple(t.to(out_dev) for t in ts)
    return ConceptDBComparison(
        layers_a=names_a, layers_b=names_b, sizes_a=sizes_a, sizes_b=sizes_b,
        pairs={key: to(ab + ba) for key, (ab, ba) in pairs.items()},
        best_ab=[to(t) for t in best_ab], best_ba=[to(t) for t in best_ba],
    )


# ------------------------------------------------------------------------------------------------
# audit: per-set best cosine of named text-concept sets, without the (prompts, components) matrix (K6 tiles + K22)
# ------------------------------------------------------------------------------------------------
@dataclass
class ConceptAudit:
    """What ``audit_concepts`` returns.  Every tensor lives on the DB's device (its layer's, for a dict DB).

    * ``sets``: the set names; ``prompts``: all prompts, set-major; ``set_offsets``: ``G + 1`` offsets into ``prompts``.
    * ``layers``: the layer names (``[None]`` for a tensor DB).
    * ``alignment[layer]``: ``(G, C)`` float32, row ``g`` = every component's best cosine over set ``g``'s prompts;
      ``best_prompt[layer]``: ``(G, C)`` int64, the index into ``prompts`` of the prompt that has it.

    ``margin`` / ``flag`` / ``rank`` take set names (one or a list) for ``valid`` and ``spurious``; a NaN alignment (a NaN in an
    embedding) propagates into the margin."""

    sets: list
    prompts: list
    set_offsets: list
    layers: list
    alignment: dict
    best_prompt: dict

    def _rows(self, names) -> list[int]:
        names = [names] if isinstance(names, str) or not isinstance(names, (list, tuple)) else list(names)
        if not names:
            raise ValueError("at least one set name is needed")
        for name in names:
            if name not in self.sets:
                raise KeyError(name)
        return [self.sets.index(name) for name in names]

    def _best(self, layer, rows: list[int]) -> torch.Tensor:
        return torch.amax(self.alignment[layer][rows], dim=0)

    def margin(self, valid, spurious) -> dict:
        """``{layer: (C,) float32}``: the best alignment over the ``spurious`` sets minus the best over the ``valid`` sets."""
        v, s = self._rows(valid), self._rows(spurious)
        return {layer: self._best(layer, s) - self._best(layer, v) for layer in self.layers}

    def flag(self, valid, spurious, margin: float = 0.0, min_alignment: float | None = None) -> dict:
        """``{layer: bool (C,)}``: ``margin(valid, spurious) > margin``, and with ``min_alignment`` also a spurious alignment of
        at least that.  A NaN margin or alignment flags nothing (every comparison with a NaN is false)."""
        v, s = self._rows(valid), self._rows(spurious)
        out = {}
        for layer in self.layers:
            best_s = self._best(layer, s)
            mask = (best_s - self._best(layer, v)) > margin
            if min_alignment is not None:
                mask &= best_s >= min_alignment
            out[layer] = mask
        return out

    def rank(self, valid, spurious, k: int = 20, importance=None):
        """The ``k`` components with the largest ``importance * margin`` across all layers: ``(values (k,), layer_index (k,),
        component (k,))``.  ``importance``: a ``(C,)`` tensor (every layer) or a dict of them per layer — a classifier row for
        the last layer, say; a layer missing from the dict counts as 1.  Order: NaN first, then the larger value, ties by the
        earlier layer and then the smaller component; ``k`` beyond the number of components is clipped."""
        k = operator.index(k)
        if k < 1:
            raise ValueError(f"k = {k} must be at least 1")
        margins = self.margin(valid, spurious)
        scores = []
        for layer in self.layers:
            m = margins[layer]
            w = importance.get(layer) if isinstance(importance, dict) else importance
            if w is not None:
                w = torch.as_tensor(w)
                if tuple(w.shape) != tuple(m.shape):
                    raise ValueError(f"importance of layer {layer!r} has shape {tuple(w.shape)}, the layer has {m.shape[0]} components")
                m = m * w.to(device=m.device, dtype=m.dtype)
            scores.append(m)
        dev = scores[0].device
        flat = torch.cat([s.to(dev) for s in scores])
        vals, order = torch.sort(flat, descending=True, stable=True)  # torch sorts NaN as the largest
        k = min(k, flat.numel())
        layer_index, component = _decode_layers(order[:k], [s.numel() for s in scores])
        return vals[:k], layer_index, component

    def describe(self, layer, component: int) -> list:
        """``[(set name, alignment, prompt string)]`` of one component, in the order of ``sets`` (a host list)."""
        vals = self.alignment[layer][:, component].tolist()
        ids = self.best_prompt[layer][:, component].tolist()
        return [(name, v, self.prompts[i] if i >= 0 else None) for name, v, i in zip(self.sets, vals, ids)]


def _check_concept_sets(concept_sets):
    """``(names, flat set-major prompts, G + 1 offsets)`` of a non-empty mapping of names to non-empty lists of strings."""
    if not isinstance(concept_sets, Mapping) or len(concept_sets) == 0:
        raise ValueError("concept_sets must be a non-empty mapping of set names to lists of prompts")
    names, prompts, offsets = [], [], [0]
    for name, members in concept_sets.items():
        if isinstance(members, str) or not isinstance(members, (list, tuple)) or len(members) == 0:
            raise ValueError(f"concept set {name!r} must be a non-empty list of strings")
        for p in members:
            if not isinstance(p, str):
                raise ValueError(f"concept set {name!r} holds {p!r}, which is not a string")
        names.append(name)
        prompts.extend(members)
        offsets.append(len(prompts))
    return names, prompts, offsets


@torch.no_grad()
def probe_setmax(query_embeds: torch.Tensor, set_offsets, aggregated_concept_db, chunk_rows: int | None = None):
    """Per set of query vectors and per component, the best cosine over the set and the query that has it, for callers who bring
    their own vectors: ``(values (G, C) float32, ids (G, C) int64)`` with ``ids`` indexing ``query_embeds``, or a dict of such
    pairs for a dict DB.  ``query_embeds (P, D)`` is set-major, set ``g`` being rows ``set_offsets[g]:set_offsets[g + 1]``; an
    empty set holds ``-inf`` / ``-1``.  The ``(P, C)`` matrix is never formed (``_native.setmax_probe``: K6 tiles + K22).
    Results live on the DB's device."""
    names, layers, is_dict = _db_layers(aggregated_concept_db)
    _check_width(query_embeds, layers)
    N.check_set_offsets(set_offsets, query_embeds.shape[0])
    probe = lambda ld, q: N.setmax_finish(N.setmax_probe(q, set_offsets, ld, chunk_rows))  # noqa: E731
    return _probe_layers(names, layers, is_dict, query_embeds, probe)


@torch.no_grad()
def audit_concepts(fm, concept_sets, aggregated_concept_db, templates: list[str] | None = None, batch_size: int | None = None,
                   chunk_size: int | None = None) -> ConceptAudit:
    """Audit a concept DB against named sets of text concepts — for a class, what the model should rely on ("valid") and what it
    should not ("spurious"): for every component its alignment with each set (the best cosine over the set's prompts), the
    prompt that gives it, and through ``ConceptAudit.margin`` / ``flag`` / ``rank`` the components that follow a spurious set
    more than a valid one.

    ``concept_sets`` is an ordered mapping ``{set name: [prompt, ...]}``.  The prompts are embedded ``chunk_size`` at a time
    (default ``LABEL_CHUNK_WORDS``; ``batch_size`` is the text tower's batch) with ``label_components``' template convention —
    each prompt's mean over ITS OWN templates minus the empty-template embedding — and each chunk is folded into every layer's
    ``(G, C)`` state (``_native.setmax_probe``) before the next is embedded; a set may straddle chunks.  Neither the
    ``(prompts, components)`` matrix nor, for ``chunk_size`` below the prompt count, all embeddings are ever resident.  A prompt
    that occurs in two sets is embedded twice.

    The sets, ``chunk_size`` and the DB's shape are checked before anything runs; as in ``label_components`` a ``D`` mismatch
    raises ``ValueError`` only after the first chunk has been embedded."""
    sets, prompts, offsets = _check_concept_sets(concept_sets)
    names, layers, _ = _db_layers(aggregated_concept_db)
    chunks = _embedded_chunks(fm, prompts, layers, templates, batch_size, chunk_size)
    dbs = [N._f32c(layer) for layer in layers]  # raises without a HIP device, before the text tower runs
    states = [None] * len(dbs)
    for start, stop, embeds in chunks:
        local = [min(max(o, start), stop) - start for o in offsets]  # the chunk's slice of every set (most are empty)
        for i, db in enumerate(dbs):
            states[i] = N.setmax_probe(embeds.to(db.device), local, db, id_base=start, state=states[i])
    alignment, best_prompt = {}, {}
    for name, layer, state in zip(names, layers, states):
        vals, ids = N.setmax_finish(state)
        alignment[name], best_prompt[name] = vals.to(layer.device), ids.to(layer.device)
    return ConceptAudit(sets=sets, prompts=prompts, set_offsets=offsets, layers=names, alignment=alignment, best_prompt=best_prompt)


class Lens:
    """Holds the foundation model and wraps the workflow (reference: lens.py:217-480)."""

    def __init__(self, fm, device=None):
        self.fm = fm
        self.device = device or self.fm.device
        self.fm.to(self.device)
        if not hasattr(self.fm, "name"):
            self.fm.name = get_fallback_name(self.fm)
            logger.debug(f"Assigned fallback name to foundation model: {self.fm.name}")

    def compute_concept_db(self, cv: AbstractComponentVisualizer, **kwargs) -> dict[str, torch.Tensor]:
        """Build the concept DB through ``cv``, or load it from ``cv``'s cache directory.

        Cache file: ``<storage_dir>/concept_database/<fm.name>/concept_db-<metadata values except
        dataset,model joined by '-'>.safetensors`` (lens.py:308-316).  ``crop=True`` (with ``crop_th``,
        ``kernel_size``, ``token_grid``, ``prefix_tokens``) builds the DB from heatmap-cropped reference samples
        (DESIGN.md §K14); its file stem ends in ``-crop-th<crop_th>-k<kernel_size>``.
        """
        if not cv.caching:
            return cv._compute_concept_db(self.fm, **kwargs)
        crop = bool(kwargs.get("crop", False))
        if crop:
            N.check_crop_args(kwargs.get("crop_th", 0.01), kwargs.get("kernel_size", 51))
        path = self._concept_db_path(cv, crop=crop, crop_th=kwargs.get("crop_th", 0.01), kernel_size=kwargs.get("kernel_size", 51))
        if path.exists():
            logger.debug(f"concept DB read from {path}")
            return load_file(filename=path)
        concept_db = cv._compute_concept_db(self.fm, **kwargs)
        save_file(tensors=concept_db, filename=path)
        logger.debug(f"concept DB written to {path}")
        return concept_db

    def _concept_db_path(self, cv, crop: bool = False, crop_th: float = 0.01, kernel_size: int = 51):
        """The cache file of ``cv``'s concept DB under this foundation model; creates its directory."""
        folder = cv.storage_dir / "concept_database" / self.fm.name
        folder.mkdir(parents=True, exist_ok=True)
        tags = [value for key, value in cv.metadata.items() if key not in ("dataset", "model")]
        stem = "concept_db-" + "-".join(tags)
        if crop:
            stem += f"-crop-th{crop_th:g}-k{kernel_size}"
        return folder / (stem + ".safetensors")

    def text_probing(self, query, aggregated_concept_db, templates=None, batch_size=None):
        return text_probing(self.fm, query, aggregated_concept_db, templates, batch_size)

    def image_probing(self, query, aggregated_concept_db):
        return image_probing(self.fm, query, aggregated_concept_db)

    def label_components(self, vocabulary, aggregated_concept_db, k=5, templates=None, batch_size=None, chunk_size=None):
        return label_components(self.fm, vocabulary, aggregated_concept_db, k, templates, batch_size, chunk_size)

    def label_distribution(self, vocabulary, aggregated_concept_db, k=5, logit_scale=100.0, templates=None, batch_size=None,
                           chunk_size=None):
        return label_distribution(self.fm, vocabulary, aggregated_concept_db, k, logit_scale, templates, batch_size, chunk_size)

    def label_rank(self, vocabulary, aggregated_concept_db, targets, templates=None, batch_size=None, chunk_size=None, logit_scale=None):
        return label_rank(self.fm, vocabulary, aggregated_concept_db, targets, templates, batch_size, chunk_size, logit_scale)

    def decompose_components(self, vocabulary, aggregated_concept_db, n_terms=4, templates=None, batch_size=None, chunk_size=None,
                             min_correlation=0.0, chunk_rows=None):
        return decompose_components(self.fm, vocabulary, aggregated_concept_db, n_terms, templates, batch_size, chunk_size,
                                    min_correlation, chunk_rows)

    def label_components_csls(self, vocabulary, aggregated_concept_db, k=5, neighbours=10, templates=None, batch_size=None,
                              chunk_size=None, chunk_rows=None):
        return label_components_csls(self.fm, vocabulary, aggregated_concept_db, k, neighbours, templates, batch_size, chunk_size,
                                     chunk_rows)

    def search_components(self, query, aggregated_concept_db, k=10, templates=None, batch_size=None):
        return search_components(self.fm, query, aggregated_concept_db, k, templates, batch_size)

    def search_components_image(self, query, aggregated_concept_db, k=10):
        return search_components_image(self.fm, query, aggregated_concept_db, k)

    def label_facets(self, vocabulary, facets, k=5, templates=None, batch_size=None, chunk_size=None):
        return label_facets(self.fm, vocabulary, facets, k, templates, batch_size, chunk_size)

    def search_facets(self, query, facets, k=10, templates=None):
        return search_facets(self.fm, query, facets, k, templates)

    def compare_concept_dbs(self, aggregated_concept_db_a, aggregated_concept_db_b, chunk_rows=None):
        return compare_concept_dbs(aggregated_concept_db_a, aggregated_concept_db_b, chunk_rows)

    def audit_concepts(self, concept_sets, aggregated_concept_db, templates=None, batch_size=None, chunk_size=None):
        return audit_concepts(self.fm, concept_sets, aggregated_concept_db, templates, batch_size, chunk_size)

    @staticmethod
    def _per_layer(fn, db):
        if isinstance(db, torch.Tensor):
            return fn(db)
        return {key: fn(value) for key, value in db.items()}

    def eval_clarity(self, concept_db):
        """``clarity_score`` of a ``(C, n, D)`` tensor or of each layer of a dict (lens.py:391-419)."""
        if isinstance(concept_db, dict) and len(concept_db) > 1:
            # the per-layer loop of lens.py:391-419 as one launch over all layers (K7 reads C*n*D*4 bytes once; a layer alone is
            # a few MB — launch-latency-sized); same values as layer by layer
            keys = list(concept_db)
            if all(isinstance(concept_db[k_], torch.Tensor) for k_ in keys):
                outs = N.clarity_multi([concept_db[k_] for k_ in keys])
                if outs is not None:
                    return {k_: o.to(concept_db[k_].device) for k_, o in zip(keys, outs)}
        return self._per_layer(clarity_score, concept_db)

    def eval_redundancy(self, aggregated_concept_db):
        """``redundancy_score`` of a ``(C, D)`` tensor or dict of tensors (lens.py:421-449)."""
        return self._per_layer(redundancy_score, aggregated_concept_db)

    def eval_redundancy_groups(self, aggregated_concept_db, threshold=0.9, **kwargs):
        """``redundancy_groups`` of a ``(C, D)`` tensor or of each layer of a dict: a ``RedundancyGroups`` or a dict of them.
        The keywords (``cohesion``, ``chunk_rows``, ``chunk_cols``) are forwarded."""
        return self._per_layer(lambda db: redundancy_groups(db, threshold=threshold, **kwargs), aggregated_concept_db)

    def eval_polysemanticity(self, concept_db):
        """``polysemanticity_score`` of a ``(C, n, D)`` tensor or dict of tensors (lens.py:451-480)."""
        return self._per_layer(polysemanticity_score, concept_db)

    def eval_facets(self, concept_db, n_clusters=2, **kwargs):
        """``polysemanticity_facets`` of a ``(C, n, D)`` tensor or of each layer of a dict: a ``Facets`` or a dict of them.
        ``n_clusters="auto"`` and the keywords (``max_clusters``, ``min_silhouette``, ``metric``, ...) are forwarded."""
        return self._per_layer(lambda V: polysemanticity_facets(V, n_clusters=n_clusters, **kwargs), concept_db)
