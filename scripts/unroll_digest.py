"""SHA-256 digests of what the trainer's HIP convs and the fused unroll compute
at the project's own edge shapes: the record a refactor of csrc/mzgo_train.hip,
csrc/mzgo_unroll.hip or csrc/mzgo_conv_bf16.hip compares with its parent's
(same inputs, same bits).  Run it on a build of the parent commit and on the
changed tree; the two JSON files must be identical.  A differing digest means
an order of summation moved.  An intended change of tiling moves them too:
nothing pins these files in the test suite.

Cases (the lists are imported from the tests, the inputs come from their
seeded CPU ``torch.Generator``s):

* unroll_fp32 / ...   the whole unroll in fp32, three head outputs and 22
                      gradients: CASES and WIDE_CASES of
                      tests/test_gpu_unroll_edges.py and the K = 0 case of
                      tests/test_gpu_unroll.py;
* unroll_bf16 / ...   the same in bf16: F64_CASES + [WIDE_CASE] of
                      tests/test_gpu_unroll_bf16.py;
* layer_fp32 / ...    mzgo_conv3x3_relu_forward, mzgo_conv3x3_backward (without
                      and with the embedding, and with a null grad_x) and
                      mzgo_dyn_conv_backward at CASES of
                      tests/test_gpu_conv_f64.py;
* layer_bf16 / ...    the bf16 entry points at CASES of
                      tests/test_gpu_conv_bf16.py.

Usage (GPU box): python scripts/unroll_digest.py [out.json] -> the JSON object
{case: {tensor: sha256}} (also written to out.json when given).
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def sha(t):
    if t is None:
        return None
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def unroll_digest(out, grads):
    assert len(grads) == 22
    d = {name: sha(t) for name, t in zip(("logits", "value", "reward"), out)}
    d.update({k: sha(g) for k, g in sorted(grads.items())})
    return d


def main():
    import test_gpu_conv_bf16 as lb
    import test_gpu_conv_f64 as lf
    import test_gpu_unroll as un
    import test_gpu_unroll_bf16 as ub
    import test_gpu_unroll_edges as ue
    from mzgo.trainer import conv3x3_backward_hip, conv3x3_forward_hip, dyn_conv_backward_hip
    name = lambda case: "x".join(str(v) for v in case)
    res = {}

    k0 = un.CASES[4]
    assert k0 == (5, 32, 1, 0, 26)
    for case in ue.CASES + [c + (2,) for c in ue.WIDE_CASES] + [k0 + (0,)]:
        out, _, grads = ue._run_unroll(*case)
        res["unroll_fp32/" + name(case)] = unroll_digest(out, grads)
    for case in ub.F64_CASES + [ub.WIDE_CASE]:
        out, _, grads = ub.run_unroll(*case, "bf16")
        res["unroll_bf16/" + name(case)] = unroll_digest(out, grads)

    for case in lf.CASES:
        N, Cin, Cout, B = case
        c = {k: v.cuda() for k, v in lf.make_case(*case).items()}
        x, w, bias, g, emb, action = c["x"], c["w"], c["bias"], c["g"], c["emb"], c["action"]
        d = {}
        y = conv3x3_forward_hip(x, w, bias)
        ye = lf._forward_hip(x, w, bias, action, emb)
        d["y"], d["y_emb"] = sha(y), sha(ye)
        for tag, got in (("", conv3x3_backward_hip(g, y, x, w)),
                         ("_emb", conv3x3_backward_hip(g, ye, x, w, action, emb)),
                         ("_nogx", conv3x3_backward_hip(g, y, x, w, need_input_grad=False)),
                         ("_dyn", dyn_conv_backward_hip(g, ye, x, action, emb, w)
                          if Cin == Cout and Cin % 16 == 0 else None)):
            if got is not None:
                d.update({k + tag: sha(v) for k, v in zip(("gx", "gw", "gb"), got)})
        res["layer_fp32/" + name(case)] = d

    for case in lb.CASES:
        c = {k: None if v is None else v.cuda() for k, v in lb.make_case(*case).items()}
        d = {"y": sha(lb.forward(c))}
        d.update({k: sha(v) for k, v in zip(("gx", "gw", "gb"), lb.backward(c))})
        d.update({k + "_nogx": sha(v) for k, v in zip(("gx", "gw", "gb"), lb.backward(c, need_gx=False))})
        res["layer_bf16/" + name(case)] = d

    torch.cuda.synchronize()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
