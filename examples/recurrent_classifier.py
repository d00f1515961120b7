"""Recurrent MNIST classifier on the HIP path -- the module graph of the reference's examples/recurrent_digits_classifier.ipynb
(cell 2): LSTM(28, 128, all) -> LSTM(128, 128, last) -> Linear(128, 10) -> Sigmoid, MSELoss, Adam; the 28 image rows are the
timesteps.  `python examples/recurrent_classifier.py --steps 50` trains it on synthetic digits (one bright bar per class position);
--graphed replays every step from a captured hipGraph (neunet_hip.graph.GraphedTrainStep)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip  # noqa: E402,F401
import neunet_hip.nn as nn  # noqa: E402


class RecurrentClassifier(nn.Module):
    def __init__(self, hidden=128):
        super().__init__()
        self.lstm1 = nn.LSTM(28, hidden, return_sequences=True)
        self.lstm2 = nn.LSTM(hidden, hidden, return_sequences=False)
        self.fc1 = nn.Linear(hidden, 10)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        x = self.lstm1(x)
        x = self.lstm2(x)
        x = x.reshape(x.shape[0], -1)
        x = self.fc1(x)
        return self.sigmoid(x)


def synthetic_batch(rng, batch):
    import numpy as np
    y = rng.integers(0, 10, batch)
    x = rng.standard_normal((batch, 28, 28)).astype(np.float32) * 0.1
    for i, c in enumerate(y):                          # class c = a bright 4-row bar starting at row 2 + 2c
        x[i, 2 + 2 * c:6 + 2 * c, 4:24] += 1.0
    return x, np.eye(10, dtype=np.float32)[y], y


def main():
    import argparse

    import numpy as np
    import torch
    from neunet_hip import Tensor
    from neunet_hip.optim import Adam
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--graphed", action="store_true", help="replay each step from a captured hipGraph")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    np.random.seed(0)
    model = RecurrentClassifier().to("cuda")
    opt = Adam(model.parameters(), lr=args.lr)
    loss_fn = nn.MSELoss()
    x0, t0, _ = synthetic_batch(rng, args.batch)
    xb, tb = Tensor(x0, device="cuda", requires_grad=False), Tensor(t0, device="cuda", requires_grad=False)
    holder = {}

    def fb():
        out = model(xb)
        holder["out"] = out
        loss = loss_fn(out, tb)
        loss.backward()
        return loss

    step_fn = None
    if args.graphed:
        from neunet_hip.distributed import GradBucket
        from neunet_hip.graph import GraphedTrainStep
        step_fn = GraphedTrainStep(fb, opt, GradBucket(model.parameters()), warmup=2)
    for step in range(args.steps):
        x, t, y = synthetic_batch(rng, args.batch)
        xb.data.copy_(torch.from_numpy(x).cuda())
        tb.data.copy_(torch.from_numpy(t).cuda())
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
    if step_fn is not None:
        step_fn.release()


if __name__ == "__main__":
    main()
