"""K11 bit-equality check: this tree's native towers (foundation_models/native_clip.py over csrc/encoder*.hip) against a tree
of another commit (``--parent-tree``: a checkout with its library built).  Each tree runs in a child process of its own,
because the two libraries export the same names.

A child builds every case below (the synthetic CLIP, the open_clip layouts of ``tests/openclip_like.py``, the RN50 attention-pool
head on a seeded map, both SigLIP layouts, ``NativeTextClip``; small geometries) in both ``gemm`` modes, with ``pool_shortcut`` /
``truncate`` on and off where the towers have them, at batch sizes 1 and 5.  It wraps the K11 functions of ``_native`` to log
every call (name, operand shapes, ``act``, which of residual / scatter / rowadd / out are given, fp32 or split result) and dumps
``encode_image`` / ``encode_text``.  The parent process compares the features with ``np.array_equal`` and the call logs entry
by entry.

    python tools/encoder_ab.py --parent-tree DIR [--out profiles/k11_tower_refactor_ab.txt]

``--wall``: the A/B of library builds this tool began as (set SEMANTICLENS_AMD_LIB): wall per ViT-B/32 image encode at B = 256.
"""
from __future__ import annotations

import argparse
import inspect
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LOGGED = ("linear", "linear3", "layernorm", "attention", "attention_pool", "attention_pool_q", "patchify", "broadcast_row",
          "embed_tokens", "tokens_from_map", "gather_rows")
PROMPTS = ["a photo of a cat", "dog", "a very long prompt with many many words in it " * 3, "two red wheels on a cart", ""]
SMALL = dict(embed_dim=64, image_size=64, patch=16, v_width=128, v_layers=2, v_heads=2, ctx=16, vocab=1000, t_width=128, t_layers=2, t_heads=2)
CLIP_VARIANTS = {
    "tok": dict(),
    "avg": dict(pool_type="avg"),
    "final_ln_after_pool+no_ln_pre+text-last": dict(pool_type="avg", no_ln_pre=True, final_ln_after_pool=True, text_pool_type="last",
                                                    no_causal_mask=True),
    "text-first+layerscale+projbias": dict(ls_init_value=0.1, proj_bias=True, text_pool_type="first"),
    "quickgelu": dict(quick_gelu=True),
    "head_dim80/32": dict(v_width=160, t_width=64, t_layers=1),
}
SIGLIP_HF = dict(width=144, layers=2, heads=2, mlp=288, image_size=64, patch=16, ctx=16, vocab=1000)  # head_dim 72
SIGLIP_OC = {
    "timm": dict(embed_dim=128, image_size=64, patch=16, width=128, layers=2, heads=2, ctx=16, vocab=1000),
    "timm-head_dim72-patch14": dict(embed_dim=144, image_size=56, patch=14, width=144, layers=2, heads=2, ctx=16, vocab=1000),
    "timm+final-linear": dict(embed_dim=96, image_size=64, patch=16, width=128, layers=1, heads=4, ctx=8, vocab=500, proj="linear",
                              init_values=0.2),
}


def install_log(N, log):
    """Wraps the K11 functions of ``_native`` (and ``Split.of``) so that every call appends one JSON-able entry to ``log``."""
    import torch

    def describe(v):
        if isinstance(v, torch.Tensor):
            return ["f32" if v.dtype == torch.float32 else str(v.dtype), list(v.shape)]
        if isinstance(v, N.Split):
            return ["split", list(v.shape)]
        return list(v) if isinstance(v, tuple) else v

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def logged(*a, **k):
            out = fn(*a, **k)
            given = {p: describe(v) for p, v in sig.bind(*a, **k).arguments.items() if v is not None and v is not False}
            if given.get("act") == 0:
                del given["act"]  # SL_ACT_NONE is the default
            log.append([name, given, describe(out)[0] if out is not None else None])
            return out

        return logged

    for name in LOGGED:
        setattr(N, name, wrap(name, getattr(N, name)))
    plain_of = N.Split.of.__func__
    logged_of = wrap("Split.of", lambda x, row_scale=None: plain_of(N.Split, x, row_scale))
    N.Split.of = classmethod(lambda cls, x, row_scale=None: logged_of(x, row_scale))


def child(args):
    sys.path.insert(0, str(Path(args.tree).resolve()))
    sys.path.append(str(ROOT / "tests"))  # openclip_like.py: the model definitions are inputs, the same file for both trees
    import torch

    from semanticlens_amd import _native as N

    log: list = []
    install_log(N, log)  # native_clip looks every one of these up on the module at call time
    import openclip_like as oc
    import synth
    from semanticlens_amd.foundation_models.native_clip import NativeClip, NativeSigLip, NativeTextClip

    dev = N.default_device()

    class Wrapped:
        def __init__(self, model, ctx, vocab, eot):
            self.model, self.name = model.to(dev).eval(), type(model).__name__
            self._tok, self._ctx = oc._tokenizer(vocab, eot=eot), ctx

        def to(self, device):
            return self.model.to(device)

        def tokenize(self, txt, context_length=None):
            return self._tok(txt, context_length=context_length or self._ctx).to(dev)

        def preprocess(self, img):
            return img

        def encode_image(self, img):
            return self.model.encode_image(img)

    def mobile_like(custom_text):
        torch.manual_seed(7)
        text = oc.TextTransformer(context_length=16, vocab_size=1000, width=128, heads=2, layers=2, output_dim=64)
        conv = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3, 2, 1), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(16, 64))
        model = oc.CustomTextCLIP(conv, text) if custom_text else oc.build_clip_vit(**SMALL)
        if not custom_text:
            model.visual = conv
        oc._randomize(model, 7)
        return Wrapped(model, 16, 1000, eot=999)

    # name -> (constructor of the base model, native class, image size or None for "no native image tower")
    synth_small = {k: v for k, v in SMALL.items() if k != "vocab"}  # synth's tokenizer draws from CLIP's 49 408 ids
    cases = {"synth-clip": (lambda: synth.SyntheticClip(device=dev, seed=3, **synth_small), NativeClip, 64)}
    for v, extra in CLIP_VARIANTS.items():
        cfg = {**SMALL, **extra}
        cases[f"open_clip-vit[{v}]"] = (lambda cfg=cfg: Wrapped(oc.build_clip_vit(seed=3, **cfg), cfg["ctx"], cfg["vocab"], cfg["vocab"] - 1), NativeClip, 64)
    cases["clip-rn50-head"] = (lambda: synth.SyntheticClipRN50(device=dev, seed=4, ctx=16, t_width=128, t_layers=2, t_heads=2), NativeClip, "map")
    cases["siglip-transformers"] = (lambda: synth.SyntheticSigLip(device=dev, seed=3, **SIGLIP_HF), NativeSigLip, 64)
    for v, geom in SIGLIP_OC.items():
        cases[f"siglip-open_clip[{v}]"] = (lambda geom=geom: Wrapped(oc.build_siglip2(seed=4, **geom), geom["ctx"], geom["vocab"], None), NativeSigLip,
                                           geom["image_size"])
    cases["text-clip[custom_text]"] = (lambda: mobile_like(True), NativeTextClip, None)
    cases["text-clip[clip]"] = (lambda: mobile_like(False), NativeTextClip, None)

    dump, logs = {}, {}
    for name, (build, cls, image) in cases.items():
        base = build()
        for gemm in ("bf16x3", "f32"):
            nat = cls(base, gemm=gemm)
            switches = [s for s in ("pool_shortcut", "truncate") if hasattr(nat.text, s)]
            for fast in ((True, False) if switches else (True,)):
                for tower in (nat.text, getattr(nat, "vision", None)):
                    for s in ("pool_shortcut", "truncate"):
                        if hasattr(tower, s):
                            setattr(tower, s, fast)
                for B in (1, 5):
                    key = f"{name}|{gemm}|{'shortcuts' if fast else 'no-shortcuts'}|B={B}"
                    del log[:]
                    g = torch.Generator().manual_seed(11)  # host generator: the same inputs in both children
                    if image == "map":  # the head on a seeded trunk map: MIOpen's convolutions are not run-to-run deterministic
                        feat = nat.vision.head((torch.rand(B, 2048, 7, 7, generator=g) * 4).to(dev))
                    elif image is not None:
                        feat = nat.encode_image(torch.randn(B, 3, image, image, generator=g).to(dev))
                    if image is not None:
                        dump[key + "|image"] = feat.cpu().numpy()
                    dump[key + "|text"] = nat.encode_text(base.tokenize(PROMPTS[:B])).cpu().numpy()
                    logs[key] = list(log)
    torch.cuda.synchronize()
    np.savez(args.dump, **dump)
    Path(args.dump + ".json").write_text(json.dumps(logs))


def wall():
    import time

    import torch

    sys.path.insert(0, str(ROOT))
    import synth
    from semanticlens_amd.foundation_models.native_clip import NativeClip

    fm = NativeClip(synth.SyntheticClip(device="cuda:0"))
    img = torch.randn(256, 3, 224, 224, device="cuda:0")
    for _ in range(5):
        fm.encode_image(img)
    best = 1e9
    for rep in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(20):
            fm.encode_image(img)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t) / 20 * 1e3)
    print(f"image B=256: {best:.3f} ms per encode (best of 5 x 20)")


def run_child(tree, path):
    subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--tree", str(tree), "--dump", str(path)], check=True,
                   timeout=900)
    return np.load(path), json.loads(Path(str(path) + ".json").read_text())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--wall", action="store_true", help="time this tree's ViT-B/32 image tower instead")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=str(ROOT), help=argparse.SUPPRESS)
    ap.add_argument("--dump", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.wall:
        return wall()
    if not args.parent_tree:
        ap.error("--parent-tree is required")
    with tempfile.TemporaryDirectory() as tmp:
        old, old_log = run_child(args.parent_tree, str(Path(tmp) / "parent.npz"))
        new, new_log = run_child(ROOT, str(Path(tmp) / "this.npz"))
    lines, bad = [], 0
    n_calls = 0
    if sorted(old.files) != sorted(new.files) or sorted(old_log) != sorted(new_log):
        lines.append("the two trees ran DIFFERENT sets of cases")
        bad += 1
    for key in sorted(new_log):
        feats = [f for f in new.files if f.startswith(key + "|")]
        same = all(f in old.files and np.array_equal(old[f], new[f]) and np.isfinite(new[f]).all() for f in feats)
        a, b = old_log.get(key, []), new_log[key]
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        n_calls += len(b)
        bad += (not same) + (first is not None)
        line = f"{key}: {', '.join(f.rsplit('|', 1)[1] + ' ' + 'x'.join(map(str, new[f].shape)) for f in feats)} {'bit-equal' if same else 'DIFFERENT'}; "
        line += f"{len(b)} calls, log equal" if first is None else f"call log DIFFERS at entry {first}: parent {a[first:first + 1]} this {b[first:first + 1]}"
        lines.append(line)
    head = [f"K11 tower refactor, bit-equality against the parent tree: {len(new_log)} runs, {len(new.files)} feature matrices, {n_calls} logged calls",
            f"every feature bit-equal and every call log equal entry by entry: {'yes' if bad == 0 else 'NO'}"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
