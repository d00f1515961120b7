"""MLP vector-quantised autoencoder on the HIP path -- the VQVAE class and training step of the reference's examples/vqvae.ipynb
(cell 2): Linear / ReLU / BatchNorm1d encoder and decoder, a 2-d latent space snapped to the nearest of 100 codes,
MSE reconstruction + vq_loss + 0.25 commit_loss, Adam(lr 0.0005).

    python examples/vqvae.py --config notebook --steps 200     # 784 pixels, hidden 512 / 256, latent 2, 100 codes, batch 100
    python examples/vqvae.py --config tiny --steps 20          # the size of tests/golden/vqvae_tiny_*.npz
    python examples/vqvae.py --codebook trained --straight-through

trains on synthetic images in [0, 1] and prints the loss and steps/s.  The step runs eagerly.  The notebook's quantize (matmul, two
norm sums, argmin, an Embedding gather) is one launch here (neunet_hip.quantize) and its vq_loss + beta * commit_loss another
(neunet_hip.vq_loss).

--codebook frozen (the default) IS the notebook: its `self.codebook.weight = nnet.tensor(...)` replaces the Embedding's Parameter with a
plain tensor, and the reference's `tensor()` defaults to requires_grad=False -- so the codebook is not in parameters(), z_q does not
require a gradient, the reconstruction gradient stops at z_q, vq_loss contributes its value only and the encoder is trained by
beta * commit_loss alone.  --codebook trained makes it a Parameter: it then receives the reference's Embedding gradient (a code chosen
by several rows keeps the LAST row's).  --straight-through additionally hands the gradient of z_q to the encoder unchanged; the
notebook has no such path."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip as nnet  # noqa: E402
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip import Tensor  # noqa: E402
from neunet_hip.optim import Adam  # noqa: E402

CONFIGS = {"notebook": dict(input_size=784, latent_size=2, num_embeddings=100, hidden=(512, 256), batch=100),
           "tiny": dict(input_size=64, latent_size=2, num_embeddings=10, hidden=(48, 32), batch=12)}
device = "cuda"


class VQVAE(nn.Module):
    """The notebook's class: same attribute names and methods.  hidden = (512, 256) are the notebook's layer widths; codebook =
    "frozen" (the notebook, see the module docstring) or "trained"."""

    def __init__(self, input_size, latent_size, num_embeddings, hidden=(512, 256), codebook="frozen", straight_through=False):
        super().__init__()
        if codebook not in ("frozen", "trained"):
            raise ValueError(f"codebook must be 'frozen' or 'trained' (got {codebook!r})")
        self.input_size = input_size
        self.latent_size = latent_size
        self.num_embeddings = num_embeddings
        self.straight_through = straight_through
        h1, h2 = hidden
        self.encoder = nn.Sequential(
            nn.Linear(input_size, h1), nn.ReLU(), nn.BatchNorm1d(h1),
            nn.Linear(h1, h2), nn.ReLU(), nn.BatchNorm1d(h2),
            nn.Linear(h2, latent_size), nn.ReLU(), nn.BatchNorm1d(latent_size),
        )
        self.codebook = nn.Embedding(num_embeddings, latent_size)
        weight = Tensor(np.random.uniform(-1 / num_embeddings, 1 / num_embeddings, (num_embeddings, latent_size)).astype(np.float32),
                        requires_grad=False)
        self.codebook.weight = nn.Parameter(weight) if codebook == "trained" else weight
        self.decoder = nn.Sequential(
            nn.Linear(latent_size, h2), nn.ReLU(), nn.BatchNorm1d(h2),
            nn.Linear(h2, h1), nn.ReLU(), nn.BatchNorm1d(h1),
            nn.Linear(h1, input_size), nn.Sigmoid(),
        )
        self.loss_fn = nn.MSELoss()

    def forward(self, x):
        z_e = self.encoder(x)
        z_q, _ = self.quantize(z_e)
        x_recon = self.decoder(z_q)
        return x_recon, z_e, z_q

    def quantize(self, z):
        return nnet.quantize(z, self.codebook.weight, self.straight_through)

    def loss_function(self, x, x_recon, z_e, z_q, beta=0.25):
        recon_loss = self.loss_fn(x_recon, x)
        return recon_loss + nnet.vq_loss(z_e, z_q, beta)

    def train_step(self, in_x, out_x, optimizer):
        x_recon, z_e, z_q = self.forward(in_x)
        loss = self.loss_function(out_x, x_recon, z_e, z_q)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss

    def encode(self, x):
        z_e = self.encoder(x)
        z_q, _ = self.quantize(z_e)
        return z_q

    def decode(self, z):
        return self.decoder(z)

    def reconstruct(self, x):
        return self.forward(x)[0]


def synthetic_images(rng, batch, pixels):
    side = int(round(pixels ** 0.5))
    x = rng.uniform(0.0, 0.2, (batch, side, side))
    for i in range(batch):
        r, c = rng.integers(0, max(side - side // 3, 1), 2)
        x[i, r:r + side // 3 + 1, c:c + side // 3 + 1] += 0.8
    return x.reshape(batch, -1)[:, :pixels].astype(np.float32)


def main():
    import argparse
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="notebook")
    ap.add_argument("--codebook", choices=("frozen", "trained"), default="frozen")
    ap.add_argument("--straight-through", action="store_true")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    np.random.seed(args.seed)                                  # initial weights and the codebook come from the global NumPy RNG, as in the notebook
    rng = np.random.default_rng(args.seed)
    vqvae = VQVAE(cfg["input_size"], cfg["latent_size"], cfg["num_embeddings"], cfg["hidden"], args.codebook,
                  args.straight_through).to(device)
    optimizer = Adam(vqvae.parameters(), lr=0.0005)
    vqvae.train()
    t0 = None
    for step in range(args.steps):
        if step == min(5, args.steps - 1):
            torch.cuda.synchronize()
            t0, s0 = time.perf_counter(), step
        batch = synthetic_images(rng, cfg["batch"], cfg["input_size"])
        in_x = Tensor(batch, device=device, requires_grad=False)
        out_x = Tensor(batch, device=device, requires_grad=False)
        loss = vqvae.train_step(in_x, out_x, optimizer)
        if step % 20 == 0 or step == args.steps - 1:
            print(f"step {step:5d}  loss {loss.item():.7f}")
    torch.cuda.synchronize()
    if t0 is not None and args.steps - s0 > 0:
        print(f"{(args.steps - s0) / (time.perf_counter() - t0):.1f} steps/s (eager, {args.config}, codebook {args.codebook}"
              f"{', straight-through' if args.straight_through else ''})")


if __name__ == "__main__":
    main()
