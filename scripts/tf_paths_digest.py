"""Every route of the Transformer scorer once, at fixed seeds, as SHA-256 digests: the check that a change to the host code that plans and
drives the routes (csrc/transformer.hip, kernels.py) left every bit where it was.  Run it under two builds (SUMK_LIB_PATH names the library;
each tree's own kernels.py drives it) and compare the two outputs: every digest and every byte count must be equal.

Routes: dense scoring in fp32; dense scoring on the plane path in bf16x6 and bf16x3 with the weights' planes given (heads of 128 columns:
attention on planes too; heads of 64: the in-loop attention between plane GEMMs); dense training; stream scoring in fp32 and bf16x3; stream
training in fp32 and bf16x3.  Training runs with layer dropout 0.1 and head dropout 0.5 and digests the scores, all parameter gradients (one
digest over the parameters in kernels.transformer_param_names order) and dx.  The exact-fp32 and stream routes run D = F = 64, 2 heads, 2
layers, videos of 70, 129 and 5 frames (across a 64-row tile and a 128-row strip, and a short video), each plain, with more_residuals, and
with a positional table; the plane path D = F = 256, 2 layers, videos of 130 and 64 frames.  The size queries of the same shapes are host
arithmetic and are printed with them.
    python scripts/tf_paths_digest.py [OUT.json]"""
import hashlib, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from summarizer_amd import _lib, kernels

SMALL = dict(D=64, heads=2, layers=2, lens=[70, 129, 5])
PLANE = dict(D=256, heads=2, layers=2, lens=[130, 64])
DROP = dict(layer_dropout_p=0.1, head_dropout_p=0.5, seed=20240607)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def tensors(shape, dev):
    """x, the parameters, a positional table and dscores of one shape, from one CPU generator"""
    D, g = shape["D"], torch.Generator().manual_seed(1234 + shape["D"])
    p = {}
    for n in kernels.transformer_param_names(shape["layers"]):
        if n.endswith("norm.weight") or "norm1.weight" in n or "norm2.weight" in n:
            p[n] = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev)
        elif n.endswith("in_proj_weight"):
            p[n] = (torch.randn(3 * D, D, generator=g) / D ** 0.5).to(dev)
        elif n.endswith("in_proj_bias"):
            p[n] = (0.1 * torch.randn(3 * D, generator=g)).to(dev)
        elif n == "k2.weight":
            p[n] = (torch.randn(1, D, generator=g) / D ** 0.5).to(dev)
        elif n == "k2.bias":
            p[n] = (0.1 * torch.randn(1, generator=g)).to(dev)
        elif n.endswith("weight"):
            p[n] = (torch.randn(D, D, generator=g) / D ** 0.5).to(dev)
        else:
            p[n] = (0.1 * torch.randn(D, generator=g)).to(dev)
    R = sum(shape["lens"])
    x = torch.randn(R, D, generator=g).to(dev)
    table = (0.5 * torch.randn(max(shape["lens"]), D, generator=g)).to(dev)
    dscores = torch.randn(R, generator=g).to(dev)
    return x, p, table, dscores


def run(shape, dev, variant, training, **route):
    x, p, table, dscores = tensors(shape, dev)
    sb = kernels.SeqBatch.get(shape["lens"], dev)
    D, heads, layers = shape["D"], shape["heads"], shape["layers"]
    opts = dict(layer_eps=1e-5, final_eps=1e-5, more_residuals=variant == "more_residuals", precision=route.pop("precision", "fp32"))
    if opts["precision"] != "fp32":
        opts["wplanes"] = kernels.transformer_wplanes(p, D, D, layers, kernels.PLANES_OF[opts["precision"]])
        assert opts["wplanes"] is not None
    if training:
        opts.update(DROP)
    rows = torch.cat([torch.arange(T, dtype=torch.int32) for T in shape["lens"]]).to(dev) if variant == "pos" else None
    xin = x.clone()      # the positional add is in place
    scores, ws = kernels.transformer_forward_packed(xin, sb, p, layers, heads, D, opts, table if variant == "pos" else None, rows,
                                                    training=training, **route)
    out = {"scores": sha(scores)}
    if training:
        grads = {n: torch.zeros_like(t) for n, t in p.items()}
        route.pop("attention_precision", None)
        dx = kernels.transformer_backward_packed(xin, sb, p, grads, layers, heads, D, opts, dscores, ws, want_dx=True, **route)
        h = hashlib.sha256()
        for n in kernels.transformer_param_names(layers):
            h.update(bytes.fromhex(sha(grads[n])))
        out.update(grads=h.hexdigest(), dx=sha(dx))
    torch.cuda.synchronize()
    return out


def sizes(shape, dev):
    sb = kernels.SeqBatch.get(shape["lens"], dev)
    a = (shape["D"], shape["D"], shape["heads"], shape["layers"], sb)
    q = {"dense": kernels.transformer_workspace_bytes(*a), "dense_train": kernels.transformer_workspace_bytes(*a, training=True),
         "stream": kernels.transformer_workspace_bytes(*a, "stream"),
         "stream_split": kernels.transformer_workspace_bytes(*a, "stream", attention_precision="bf16x3"),
         "stream_train": kernels.transformer_workspace_bytes(*a, "stream", training=True),
         "stream_split_train": kernels.transformer_workspace_bytes(*a, "stream", training=True, attention_train_precision="bf16x3")}
    lib = _lib.load()
    for name, code in kernels.PRECISIONS.items():
        q["dense_for_" + name] = lib.sumk_transformer_workspace_bytes_for(*a[:4], sb.n_seq, sb.off_host_p, 0, code)
    return {k: int(v) for k, v in q.items()}


def main():
    dev = torch.device("cuda:0")
    res = {"shapes": {"small": SMALL, "plane": PLANE}, "dropout": DROP,
           "sizes": {"small": sizes(SMALL, dev), "plane": sizes(PLANE, dev), "plane_4_heads": sizes(dict(PLANE, heads=4), dev)}, "digests": {}}
    routes = {"dense_score_fp32": (False, {}), "dense_train": (True, {}),
              "stream_score_fp32": (False, dict(attention="stream")),
              "stream_score_bf16x3": (False, dict(attention="stream", attention_precision="bf16x3")),
              "stream_train_fp32": (True, dict(attention="stream")),
              "stream_train_bf16x3": (True, dict(attention="stream", attention_train_precision="bf16x3"))}
    for name, (training, route) in routes.items():
        for variant in ("plain", "more_residuals", "pos"):
            res["digests"][f"{name}/{variant}"] = run(SMALL, dev, variant, training, **route)
    for prec in ("bf16x6", "bf16x3"):
        res["digests"][f"dense_score_planes_{prec}/attention_on_planes"] = run(PLANE, dev, "plain", False, precision=prec)
        res["digests"][f"dense_score_planes_{prec}/attention_in_loop"] = run(dict(PLANE, heads=4), dev, "more_residuals", False, precision=prec)
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
