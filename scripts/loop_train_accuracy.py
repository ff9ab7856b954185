"""The two floors of tests/test_gpu_loop_train.py, measured on the GPU with nothing of the loop-head training code in the loop:
  FLOOR_OP   the dense fp32 torch formulation of loop_pool (relu(x W1^T + b1).view(B, L, E).mean(1) under autograd) against its
             fp64 run on the same inputs, over the test's shapes: worst max |g32 - g64| / max |g64| of dW1 and db1, doubled;
  FLOOR_E2E  the dense fp32 torch head + loss (tests/loop_train_restated.py), fed with the features the decoder's EVAL-mode
             trunk returns (the inference kernels), against the fixture's fp64 loss and gradients: worst error, doubled.
Prints a markdown report (kept as profiles/loop_train_accuracy.md).

  python scripts/loop_train_accuracy.py [> profiles/loop_train_accuracy.md]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch

import loop_train_cases as C
import loop_train_restated as R
from test_gpu_loop_train import POOL_SHAPES, dense_pool, pool_inputs
from test_loop_train_host import fixture_checks, rel_err
from deeppointmap_amd.decoder import Decoder

DEV = "cuda"
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    if not torch.cuda.is_available():
        sys.exit("loop_train_accuracy.py measures on a GPU; none is visible")
    torch.set_grad_enabled(False)
    n = lambda t: t.cpu().numpy()   # noqa: E731
    print("# Loop-head training: accuracy floors\n")
    print(f"`python scripts/loop_train_accuracy.py` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}).  Errors are "
          "max |got - fp64| / max |fp64| per tensor.\n")
    print("## FLOOR_OP: dense fp32 torch `loop_pool` against its fp64 run\n\n| B | L | dW1 | db1 |\n|---|---|---|---|")
    worst_op = 0.0
    for B, L in POOL_SHAPES:
        x, W1, b1, g = pool_inputs(B, L)
        _, w32, b32 = dense_pool(x, W1, b1, g, B, L, torch.float32)
        _, w64, b64 = dense_pool(x, W1, b1, g, B, L, torch.float64)
        ew, eb = rel_err(n(w32), n(w64)), rel_err(n(b32), n(b64))
        worst_op = max(worst_op, ew, eb)
        print(f"| {B} | {L} | {ew:.2e} | {eb:.2e} |")
    print(f"\nworst {worst_op:.3e}; FLOOR_OP = 2 x worst = {2 * worst_op:.2e}\n")
    print("## FLOOR_E2E: dense fp32 torch head on the eval-mode trunk's features against the fixture's fp64 run\n")
    print("| case | loss | worst gradient | its tensor | fixture's largest e |\n|---|---|---|---|---|")
    worst = 0.0
    for name, (inputs, cfg) in C.cases().items():
        fx = C.load_fixture(name, GOLDEN)
        dec = Decoder(cfg)
        dec.load_state_dict(C.state_dict(cfg), strict=True)
        dec = dec.to(DEV)
        t = lambda a: torch.from_numpy(a).float().to(DEV)   # noqa: E731
        ps, pd = (None, None) if inputs["ps"] is None else (torch.from_numpy(m).to(DEV) for m in C.masks(inputs))
        x, _, y, _, B, M, N = dec._descriptor_attention_forward(t(inputs["src"]), t(inputs["dst"]), ps, pd)
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in dec.state_dict().items() if "loop" in k}
        with torch.enable_grad():
            prob = R.loop_head(sd, x.view(B, M, -1), y.view(B, N, -1))
            loss, _ = R.loop_loss(prob, R.labels(t(inputs["src_T"]), t(inputs["dst_T"]), cfg.train.loop_detection.distance))
            loss.backward()
        pg = {k: n(v.grad) for k, v in sd.items()}
        el = abs(float(loss) - fx["loss/64"][0]) / abs(fx["loss/64"][0])
        rows = [(k, rel_err(got.reshape(want.shape), want), e)
                for k, got, want, e in fixture_checks(fx, "64", n(prob), np.zeros_like(fx["grad/dprob/64"]), pg) if k not in ("prob", "grad/dprob")]
        k, err, _ = max(rows, key=lambda r: r[1])
        worst = max(worst, err, el)
        print(f"| {name} | {el:.2e} | {err:.2e} | {k.split('loop_head.')[-1]} | {max(r[2] for r in rows):.2e} |")
    print(f"\nworst {worst:.3e}; FLOOR_E2E = 2 x worst = {2 * worst:.2e}")


if __name__ == "__main__":
    main()
