"""LeNet-5 on the HIP path: the textbook consumer of nn.ZeroPad2d, nn.AvgPool2d and nn.Flatten.  28x28x1 digits are zero-padded to
32x32; two 5x5 convolutions, each followed by Tanh and 2x2 average pooling; Flatten; Linear 400 -> 120 -> 84 -> 10 with Tanh between;
CrossEntropyLoss, Adam(lr 1e-3).  61,706 parameters.

    python examples/lenet5.py --steps 50                 # eager steps on synthetic digits (one bright blob per class position)
    python examples/lenet5.py --steps 200 --mode graph   # every step replayed from a captured hipGraph (neunet_hip.graph)
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip  # noqa: E402,F401
import neunet_hip.nn as nn  # noqa: E402


class LeNet5(nn.Module):
    def __init__(self):
        super().__init__()
        self.pad = nn.ZeroPad2d(2)
        self.conv1 = nn.Conv2d(1, 6, 5)
        self.pool1 = nn.AvgPool2d(2)
        self.conv2 = nn.Conv2d(6, 16, 5)
        self.pool2 = nn.AvgPool2d(2)
        self.flatten = nn.Flatten()
        self.fc1 = nn.Linear(400, 120)
        self.fc2 = nn.Linear(120, 84)
        self.fc3 = nn.Linear(84, 10)
        self.tanh = nn.Tanh()

    def forward(self, x):
        x = self.pad(x)
        x = self.pool1(self.tanh(self.conv1(x)))
        x = self.pool2(self.tanh(self.conv2(x)))
        x = self.flatten(x)
        x = self.tanh(self.fc1(x))
        x = self.tanh(self.fc2(x))
        return self.fc3(x)


def synthetic_batch(rng, batch):
    """Class c = a bright 6x6 blob at a class-specific position on a noisy background (examples/conv_classifier.py's digits)."""
    import numpy as np
    y = rng.integers(0, 10, batch)
    x = rng.standard_normal((batch, 1, 28, 28)).astype(np.float32) * 0.1
    for i, c in enumerate(y):
        r0, c0 = 2 + 5 * (c // 5) * 2, 1 + 5 * (c % 5)
        x[i, 0, r0:r0 + 6, c0:c0 + 6] += 1.0
    return x, y.astype(np.int32)


def main():
    import argparse

    import numpy as np
    import torch
    from neunet_hip import Tensor
    from neunet_hip.optim import Adam
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--mode", default="eager", choices=["eager", "graph"], help="graph: replay each step from a captured hipGraph")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    np.random.seed(0)
    model = LeNet5().to("cuda")
    opt = Adam(model.parameters(), lr=1e-3)
    loss_fn = nn.CrossEntropyLoss()
    x0, y0 = synthetic_batch(rng, args.batch)
    xb = Tensor(x0, device="cuda", requires_grad=False)
    yb = Tensor(y0, dtype=np.int32, device="cuda", requires_grad=False)
    holder = {}

    def fb():
        out = model(xb)
        holder["out"] = out
        loss = loss_fn(out, yb)
        loss.backward()
        return loss

    step_fn = None
    if args.mode == "graph":
        from neunet_hip.distributed import GradBucket
        from neunet_hip.graph import GraphedTrainStep
        step_fn = GraphedTrainStep(fb, opt, GradBucket(model.parameters()), warmup=2, count_nodes=True)
        print(f"captured step: {step_fn.kernel_nodes} kernel launches", flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(args.steps):
        x, y = synthetic_batch(rng, args.batch)
        xb.data.copy_(torch.from_numpy(x).cuda())
        yb.data.copy_(torch.from_numpy(y).cuda())
        if step_fn is not None:
            loss = step_fn()
        else:
            opt.zero_grad()
            loss = fb()
            opt.step()
        if step % 10 == 0 or step == args.steps - 1:
            msg = f"step {step:4d}  loss {loss.item():.4f}"
            if step_fn is None:
                msg += f"  acc {float((np.argmax(holder['out'].numpy(), 1) == y).mean()):.2f}"
            print(msg, flush=True)
    torch.cuda.synchronize()
    print(f"{args.steps / (time.perf_counter() - t0):.1f} steps/s ({args.mode}, batch {args.batch}, host batch synthesis included)")
    if step_fn is not None:
        step_fn.release()


if __name__ == "__main__":
    main()
