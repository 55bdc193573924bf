"""Records the distinct BatchNorm / split-attention / column-sum wrapper calls of ONE training step of BASELINE configs 2, 4
and 5 (bench.py's model, batch and precision), as the literal list tests/test_bn_routes_gpu.py::PRODUCTION holds.

    python tools_dev/record_bn_calls.py [--configs 2 4 5] [--out FILE]

Every kernels.<entry> the model calls is wrapped by a recorder (the model calls them as K.<entry>), one eager step runs,
and each distinct (entry, shape, storage types, flags) is printed once, in first-call order.  Needs a HIP device."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _dt(t):
    import torch
    return None if t is None else ("bf16" if t.dtype == torch.bfloat16 else "f32")


def _mc(t):
    C = t.shape[-1]
    return t.numel() // C, C


def _key(name, args, kw):
    """(entry, M or (B, HW), C, flags) -- everything that picks a route inside the library"""
    get = lambda i, k, d=None: args[i] if len(args) > i else kw.get(k, d)
    if name == "bn_stats":
        x, st = args[0], get(8, "stats")
        return (name,) + _mc(x) + ((("x", _dt(x)), ("training", bool(args[5])), ("ext_rows", st[1] if st else 0)),)
    if name == "bn_fwd":
        x, res, st = args[0], get(7, "residual"), get(10, "stats")
        fl = (("x", _dt(x)), ("y", "bf16" if str(kw.get("out_dtype", "")).endswith("bfloat16") else "f32"),
              ("training", bool(args[5])), ("relu", bool(args[6])), ("res", _dt(res)),
              ("res_bn", kw.get("residual_bn") is not None), ("ext_rows", st[1] if st else 0),
              ("mask", bool(kw.get("want_mask"))), ("planes", int(kw.get("planes", 0))),
              ("keep_f32", bool(kw.get("keep_f32", True))))
        return (name,) + _mc(x) + (fl,)
    if name == "bn_bwd":
        dy, ymask, x = args[0], args[1], args[2]
        ext = kw.get("ext")
        fl = (("dy", _dt(dy)), ("x", _dt(x)), ("dx", "bf16" if str(kw.get("dx_dtype", "")).endswith("bfloat16") else "f32"),
              ("training", bool(args[4])), ("ymask", ymask is not None), ("mask", kw.get("mask") is not None),
              ("gout", bool(get(7, "want_gout", False))), ("ext_rows", ext[1] if ext else 0))
        return (name,) + _mc(x) + (fl,)
    if name == "colsum":
        a, b = args[0], get(2, "b")
        return (name,) + _mc(a) + ((("b", b is not None), ("alpha", float(get(3, "alpha", 1.0)))),)
    if name in ("sa_gap", "sa_dattn", "sa_apply_fwd"):
        x = args[0]
        B, H, W, C2 = x.shape
        fl = (("x", _dt(x)), ("bn", get(2 if name == "sa_dattn" else 1, "bn") is not None))
        if name == "sa_dattn":
            fl += (("stats", bool(get(3, "want_stats", False))),)
        if name == "sa_apply_fwd":
            fl += (("y", "bf16" if str(kw.get("out_dtype", "")).endswith("bfloat16") else "f32"),)
        return (name, B, H * W, C2, fl)
    if name == "sa_bn_bwd":
        dout, x0 = args[0], args[3]
        B, H, W, Cp = dout.shape
        fl = (("x", _dt(x0)), ("training", bool(args[5])), ("planes", int(kw.get("planes", 0))),
              ("keep_f32", bool(kw.get("keep_f32", True))), ("sums", kw.get("sums") is not None))
        return (name, B, H * W, 2 * Cp, fl)
    raise KeyError(name)


ENTRIES = ("bn_stats", "bn_fwd", "bn_bwd", "colsum", "sa_gap", "sa_dattn", "sa_apply_fwd", "sa_bn_bwd")


def record(config):
    import torch
    import bench
    from scouter_amd import kernels as K
    from scouter_amd.sloter.slot_model import SlotModel
    cfg = dict(bench.CONFIGS[config])
    torch.manual_seed(0)
    model = SlotModel(bench.make_args(cfg)).cuda().train()
    x, y = bench.synth_batch(cfg["batch"], cfg["img_size"], cfg["num_classes"], 0, torch.device("cuda"), 3)
    seen, orig = {}, {n: getattr(K, n) for n in ENTRIES}

    def wrap(n):
        def f(*args, **kw):
            seen.setdefault(_key(n, args, kw), None)
            return orig[n](*args, **kw)
        return f
    for n in ENTRIES:
        setattr(K, n, wrap(n))
    try:
        out, losses = model(x, y)
        losses[0].backward(model.loss_seed(losses[0]))
        torch.cuda.synchronize()
    finally:
        for n in ENTRIES:
            setattr(K, n, orig[n])
    del model, out, losses
    torch.cuda.empty_cache()
    return list(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 4, 5])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    lines = []
    for c in a.configs:
        for k in record(c):
            lines.append("    (%d, %r)," % (c, k))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
