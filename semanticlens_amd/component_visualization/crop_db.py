"""Concept DBs from heatmap-cropped reference samples.

Row ``[c, j]`` of a cropped concept DB is the foundation-model embedding of reference sample
``get_max_reference(layer)[c, j]`` cropped to the box of its heatmap for component ``c``, instead of the whole image.
The pieces, per chunk of unique reference samples:

* heat + box: for the activation visualizer one forward of the chunk's ``dataset_model`` samples with hooks on every
  requested layer; K14 (``sl_activation_heat_boxes``) runs on each layer's output inside its hook, so a later in-place
  op cannot change what it reads, and the forward stops after the last hooked layer.  The relevance visualizer brings
  its conditional heatmaps and runs ``sl_heat_boxes`` on them;
* :func:`scale_box` maps a box from the model input ``(H, W)`` to the ``dataset_fm`` image;
* ROI preprocessing (``DevicePreprocess.crops``: one upload per unique sample, crop then resize on the device) or, for a
  foundation model without device preprocessing, host crops through ``fm.preprocess``;
* ``fm.encode_image`` in batches of at most ``batch_size`` pairs, scattered into the ``(C, k, D)`` buffers.

Heat and crop rules are unpinned: the upstream project names attribution-based cropping but ships no implementation.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from semanticlens_amd import _native as N

#: unique reference samples per forward of the activation path; fixed, so that the concept DB does not depend on
#: ``batch_size`` (a layer's output can differ in the last bits with the batch it was computed in)
FORWARD_CHUNK = 128


class _StopForward(Exception):
    """Raised by the last hook: nothing after the hooked layers is needed."""


def scale_box(box, model_hw, fm_hw):
    """A box (row1, row2, col1, col2) of the model input ``model_hw`` = (H, W) -> the same region of an image of
    ``fm_hw`` = (h, w) pixels: ``r1' = floor(r1 h / H)``, ``r2' = ceil(min(r2, H) h / H)`` (columns alike), clamped to
    the image.  An extent that ends up empty grows to one pixel.  The identity (up to clamping) when the sizes agree."""
    H, W = (int(v) for v in model_hw)
    h, w = (int(v) for v in fm_hw)
    r1, r2, c1, c2 = (int(v) for v in box)

    def lo(v, n, m):
        return min(max((max(v, 0) * m) // n, 0), m)

    def hi(v, n, m):
        return min(max(-((-min(v, n) * m) // n), 0), m)

    a, b, c, d = lo(r1, H, h), hi(r2, H, h), lo(c1, W, w), hi(c2, W, w)
    if b <= a:
        a = min(a, h - 1)
        b = a + 1
    if d <= c:
        c = min(c, w - 1)
        d = c + 1
    return a, b, c, d


def infer_token_grid(T: int, token_grid=None, prefix_tokens=None):
    """``(gh, gw, prefix)`` of a token layer with ``T`` tokens: as given, or inferred when ``T`` (no prefix) or
    ``T - 1`` (one class token) is a perfect square."""
    T = int(T)
    if token_grid is not None:
        gh, gw = (int(v) for v in token_grid)
        prefix = T - gh * gw if prefix_tokens is None else int(prefix_tokens)
        if gh < 1 or gw < 1 or prefix < 0 or prefix + gh * gw > T:
            raise ValueError(f"token_grid {tuple(token_grid)} with prefix_tokens {prefix} does not fit a layer of {T} tokens")
        return gh, gw, prefix
    if prefix_tokens is not None:
        n = T - int(prefix_tokens)
        g = math.isqrt(max(n, 0))
        if int(prefix_tokens) < 0 or n < 1 or g * g != n:
            raise ValueError(f"{T} tokens minus prefix_tokens={prefix_tokens} is not a square grid: pass token_grid")
        return g, g, int(prefix_tokens)
    for prefix in (0, 1):
        n = T - prefix
        g = math.isqrt(max(n, 0))
        if n >= 1 and g * g == n:
            return g, g, prefix
    raise ValueError(f"cannot infer the patch grid of a layer with {T} tokens (neither T nor T - 1 is a perfect square): "
                     "pass token_grid=(gh, gw) and prefix_tokens")


def _first(item):
    return item[0] if isinstance(item, (tuple, list)) else item


def item_hw(item):
    """(h, w) of a ``dataset_fm`` item: PIL image, (h, w[, c]) uint8 array / tensor or (C, h, w) float tensor / array."""
    if hasattr(item, "mode") and hasattr(item, "size") and not isinstance(item, (np.ndarray, torch.Tensor)):
        return item.size[1], item.size[0]
    shape = tuple(item.shape)
    if len(shape) == 2 or (len(shape) == 3 and _hwc(item)):
        return shape[0], shape[1]
    if len(shape) == 3:
        return shape[1], shape[2]
    raise ValueError(f"cannot crop a dataset_fm item of shape {shape}")


def _hwc(item) -> bool:
    return item.dtype in (np.uint8, torch.uint8) and item.shape[-1] in (1, 3, 4)


def crop_item(item, box):
    """Host crop of one ``dataset_fm`` item to ``box`` = (row1, row2, col1, col2), already clamped: PIL ``crop``, or
    slicing of HWC uint8 arrays / tensors (CHW for other 3-D arrays / tensors)."""
    r1, r2, c1, c2 = (int(v) for v in box)
    if hasattr(item, "mode") and hasattr(item, "size") and not isinstance(item, (np.ndarray, torch.Tensor)):
        return item.crop((c1, r1, c2, r2))
    if item.ndim == 2 or _hwc(item):
        return item[r1:r2, c1:c2]
    return item[:, r1:r2, c1:c2]


def _as_hwc(item):
    """A (3, h, w) uint8 array / tensor as (h, w, 3) for the device preprocess; everything else unchanged."""
    if isinstance(item, (np.ndarray, torch.Tensor)) and item.ndim == 3 and not _hwc(item) and item.shape[0] == 3:
        return item.permute(1, 2, 0) if isinstance(item, torch.Tensor) else item.transpose(1, 2, 0)
    return item


class _Scatter:
    """The ``(C * k, D)`` output buffer of each layer, allocated when the first embedding shows ``D``."""

    def __init__(self, shapes: dict):
        self.shapes = shapes
        self.bufs = {}

    def put(self, layer, rows: torch.Tensor, emb: torch.Tensor):
        emb = N.to_device(emb.detach()).to(torch.float32)
        if layer not in self.bufs:
            C, k = self.shapes[layer]
            self.bufs[layer] = torch.zeros((C * k, emb.shape[1]), dtype=torch.float32, device=emb.device)
        self.bufs[layer].index_copy_(0, rows.to(emb.device), emb)

    def result(self, keep_on_device: bool) -> dict:
        out = {}
        for layer, (C, k) in self.shapes.items():
            if layer not in self.bufs:
                continue
            t = self.bufs[layer].reshape(C, k, -1)
            out[layer] = t if keep_on_device else t.cpu()
        return out


def embed_boxed(fm, items, boxes, index, batch_size: int):
    """Embeddings ``(P, D)`` of ``items[index[j]]`` cropped to ``boxes[j]`` (clamped, in item pixels): ROI preprocessing
    on the device when ``fm`` has a ``device_preprocess``, else host crops through ``fm.preprocess``; encoded in batches
    of at most ``batch_size`` pairs."""
    P = len(index)
    pp = getattr(fm, "device_preprocess", None)
    outs = []
    if pp is not None:
        pre = pp.crops([_as_hwc(it) for it in items], boxes, index)
        for s in range(0, P, batch_size):
            outs.append(N.to_device(fm.encode_image(pre[s:s + batch_size]).detach()).to(torch.float32))
    else:
        for s in range(0, P, batch_size):
            crops = [crop_item(items[int(i)], b) for i, b in zip(index[s:s + batch_size], boxes[s:s + batch_size])]
            pre = fm.preprocess(crops)
            if torch.is_tensor(pre):
                pre = pre.to(fm.device)
            outs.append(N.to_device(fm.encode_image(pre).detach()).to(torch.float32))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def _pairs(refs: dict):
    """Referenced pairs of every layer: (layer index, flat row c * k + j, component c, sample id) as int64 arrays, and
    the rows of ``-1`` (never filled) slots per layer."""
    lay, row, comp, sid, empty = [], [], [], [], {}
    for li, ids in enumerate(refs.values()):
        ids = ids.to(torch.int64).cpu()
        C, k = ids.shape
        flat = ids.reshape(-1).numpy()
        rows = np.arange(C * k, dtype=np.int64)
        ok = flat >= 0
        lay.append(np.full(int(ok.sum()), li, dtype=np.int64))
        row.append(rows[ok])
        comp.append(rows[ok] // k)
        sid.append(flat[ok])
        empty[li] = rows[~ok]
    cat = (lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int64))
    return cat(lay), cat(row), cat(comp), cat(sid), empty


def _load_model_samples(cv, ids) -> torch.Tensor:
    return torch.stack([torch.as_tensor(_first(cv.dataset[int(i)])) for i in ids])


class _Embedder:
    """ROI + encode + scatter of boxed pairs, chunk by chunk of unique samples."""

    def __init__(self, cv, fm, refs: dict, batch_size: int):
        self.cv, self.fm, self.batch_size = cv, fm, int(batch_size)
        self.names = list(refs)
        self.scatter = _Scatter({name: tuple(ids.shape) for name, ids in refs.items()})

    def chunk(self, uniq, pos, lay, row, boxes, model_hw):
        """Pairs referring to ``uniq[pos[j]]`` with model-input ``boxes`` (P, 4) -> scattered embeddings."""
        items = [_first(self.cv.dataset_fm[int(s)]) for s in uniq]
        fm_hw = [item_hw(it) for it in items]
        scaled = np.array([scale_box(b, model_hw, fm_hw[p]) for b, p in zip(boxes, pos)], dtype=np.int32).reshape(-1, 4)
        emb = embed_boxed(self.fm, items, scaled, np.asarray(pos, dtype=np.int64), self.batch_size)
        for li, name in enumerate(self.names):
            sel = np.nonzero(lay == li)[0]
            if len(sel):
                self.scatter.put(name, torch.from_numpy(row[sel]), emb[torch.from_numpy(sel).to(emb.device)])

    def empty_slots(self, empty: dict):
        """``-1`` slots: the uncropped last sample, as the uncropped DB has there (``embeds[-1]``)."""
        if not any(len(v) for v in empty.values()):
            return
        last = len(self.cv.dataset_fm) - 1
        item = _first(self.cv.dataset_fm[last])
        h, w = item_hw(item)
        emb = embed_boxed(self.fm, [item], np.array([[0, h, 0, w]], dtype=np.int32), np.zeros(1, dtype=np.int64), 1)
        for li, name in enumerate(self.names):
            rows = empty[li]
            if len(rows):
                self.scatter.put(name, torch.from_numpy(rows), emb.expand(len(rows), -1))


def _sorted_chunks(sid, chunk):
    """Pair order sorted by sample id (stable) and the boundaries of chunks of ``chunk`` unique samples."""
    order = np.argsort(sid, kind="stable")
    uniq, first = np.unique(sid[order], return_index=True)
    bounds = [(int(first[u]), int(first[u + chunk]) if u + chunk < len(uniq) else len(order), uniq[u:u + chunk])
              for u in range(0, len(uniq), chunk)]
    return order, bounds


def forward_heat_boxes(cv, sample_ids, pairs: dict, kernel_size: int, crop_th: float, token_grid=None, prefix_tokens=None,
                       want_heat: bool = False):
    """One forward of ``dataset_model`` samples ``sample_ids`` with K14 launched in the hook of every layer of ``pairs``
    = ``{layer: (rows into sample_ids, channels)}``.  Returns ``({layer: (heat or None, box (P, 4) int32)}, (H, W))``."""
    images = N.to_device(_load_model_samples(cv, sample_ids), cv.device)
    hw = tuple(images.shape[-2:])
    N.check_crop_args(crop_th, kernel_size, *hw)
    modules = dict(cv.model.named_modules())
    out, handles = {}, []

    def hook_for(name):
        rows, chans = pairs[name]

        def hook(module, ins, o):
            if name in out:
                return
            t = o[0] if isinstance(o, (tuple, list)) else o
            grid, prefix = None, 0
            if t.ndim == 3:
                gh, gw, prefix = infer_token_grid(t.shape[1], token_grid, prefix_tokens)
                grid = (gh, gw)
            out[name] = N.activation_heat_boxes(t, rows, chans, hw, kernel_size, crop_th, token_grid=grid, prefix_tokens=prefix,
                                                want_heat=want_heat)
            if len(out) == len(pairs):
                raise _StopForward

        return hook

    for name in pairs:
        handles.append(modules[name].register_forward_hook(hook_for(name)))
    try:
        with torch.no_grad():
            cv.model(images)
    except _StopForward:
        pass
    finally:
        for h in handles:
            h.remove()
    missing = [n for n in pairs if n not in out]
    if missing:
        raise RuntimeError(f"layers {missing} did not run in the model's forward")
    return out, hw


def activation_crop_db(cv, fm, batch_size: int, keep_on_device: bool, crop_th: float, kernel_size: int, token_grid=None,
                       prefix_tokens=None) -> dict:
    """The cropped concept DB of an ``ActivationComponentVisualizer`` (after ``run()``)."""
    N.check_crop_args(crop_th, kernel_size)
    refs = {name: cv.get_max_reference(name) for name in cv.layer_names}
    lay, row, comp, sid, empty = _pairs(refs)
    n_total = len(cv.dataset_fm)
    if len(sid) and int(sid.max()) >= n_total:
        raise IndexError(f"index out of range in embeds[sample_ids] (dataset size {n_total})")
    fm.to(cv.device)
    emb = _Embedder(cv, fm, refs, batch_size)
    names = list(refs)
    order, chunks = _sorted_chunks(sid, FORWARD_CHUNK)
    for a, b, uniq in chunks:
        sel = order[a:b]
        pos = np.searchsorted(uniq, sid[sel])
        pairs = {}
        for li, name in enumerate(names):
            m = lay[sel] == li
            if m.any():
                pairs[name] = (torch.from_numpy(pos[m]), torch.from_numpy(comp[sel][m]))
        res, hw = forward_heat_boxes(cv, uniq, pairs, kernel_size, crop_th, token_grid, prefix_tokens)
        # boxes back in pair order: layer by layer as `pairs` was built
        boxes = np.zeros((len(sel), 4), dtype=np.int32)
        host = {name: res[name][1].cpu().numpy() for name in pairs}
        for li, name in enumerate(names):
            m = np.nonzero(lay[sel] == li)[0]
            if len(m):
                boxes[m] = host[name]
        emb.chunk(uniq, pos, lay[sel], row[sel], boxes, hw)
    emb.empty_slots(empty)
    return emb.scatter.result(keep_on_device)


def relevance_crop_db(cv, fm, batch_size: int, keep_on_device: bool, crop_th: float, kernel_size: int) -> dict:
    """The cropped concept DB of a ``RelevanceComponentVisualizer`` (after ``run()``): boxes of the receptive-field
    conditional relevance heatmaps of the relevance-ranked references (``compute_heatmaps(mode="relevance", rf=True)``'s
    heat, pairs batched across concepts), then the same ROI path."""
    N.check_crop_args(crop_th, kernel_size)
    refs = {name: cv.get_max_reference(name) for name in cv.layer_names}
    lay, row, comp, sid, empty = _pairs(refs)
    n_total = len(cv.dataset_fm)
    if len(sid) and int(sid.max()) >= n_total:
        raise IndexError(f"index out of range in embeds[sample_ids] (dataset size {n_total})")
    fm.to(cv.device)
    boxes = np.zeros((len(sid), 4), dtype=np.int32)
    hw = None
    for li, name in enumerate(refs):
        sel = np.nonzero(lay == li)[0]
        for s in range(0, len(sel), batch_size):
            part = sel[s:s + batch_size]
            heat = cv._conditional_heat(name, [(int(c), int(i)) for c, i in zip(comp[part], sid[part])], rf=True,
                                        batch_size=batch_size)
            hw = tuple(heat.shape[-2:])
            boxes[part] = N.heat_boxes(heat, kernel_size, crop_th).cpu().numpy()
    emb = _Embedder(cv, fm, refs, batch_size)
    order, chunks = _sorted_chunks(sid, FORWARD_CHUNK)
    for a, b, uniq in chunks:
        sel = order[a:b]
        emb.chunk(uniq, np.searchsorted(uniq, sid[sel]), lay[sel], row[sel], boxes[sel], hw)
    emb.empty_slots(empty)
    return emb.scatter.result(keep_on_device)
