"""MLP variational autoencoder on the HIP path -- the VAE class and training step of the reference's examples/vae.ipynb (cell 2):
Linear / ReLU / BatchNorm1d encoder and decoder, a 2-d latent space, BCELoss(reduction="sum") + the KL term, Adam(lr 0.0005).

    python examples/vae.py --config notebook --steps 200      # 784 pixels, hidden 512 / 256, latent 2, batch 100
    python examples/vae.py --config tiny --steps 20           # the size of tests/golden/vae_tiny.npz

trains on synthetic images in [0, 1] and prints the loss and steps/s.  The step runs eagerly.  The notebook's two latent-space
expressions, the reparameterisation and the KL term, are one launch each way here (neunet_hip.reparameterize, neunet_hip.gaussian_kld)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip as nnet  # noqa: E402
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip import Tensor  # noqa: E402
from neunet_hip.optim import Adam  # noqa: E402

CONFIGS = {"notebook": dict(input_size=784, latent_size=2, hidden=(512, 256), batch=100),
           "tiny": dict(input_size=64, latent_size=2, hidden=(48, 32), batch=12)}
device = "cuda"


class VAE(nn.Module):
    """The notebook's class: same attribute names and methods.  hidden = (512, 256) are the notebook's layer widths."""

    def __init__(self, input_size, latent_size, hidden=(512, 256)):
        super().__init__()
        self.input_size = input_size
        self.latent_size = latent_size
        h1, h2 = hidden
        self.encoder = nn.Sequential(
            nn.Linear(input_size, h1), nn.ReLU(), nn.BatchNorm1d(h1),
            nn.Linear(h1, h2), nn.ReLU(), nn.BatchNorm1d(h2),
            nn.Linear(h2, latent_size), nn.ReLU(), nn.BatchNorm1d(latent_size),
        )
        self.decoder = nn.Sequential(
            nn.Linear(latent_size, h2), nn.ReLU(), nn.BatchNorm1d(h2),
            nn.Linear(h2, h1), nn.ReLU(), nn.BatchNorm1d(h1),
            nn.Linear(h1, input_size), nn.Sigmoid(),
        )
        self.mu_encoder = nn.Linear(latent_size, latent_size)
        self.logvar_encoder = nn.Linear(latent_size, latent_size)
        self.loss_fn = nn.BCELoss(reduction="sum")

    def reparameterize(self, mu, logvar, eps=None):
        """z = mu + eps * exp(logvar / 2); eps: the standard-normal draw (the notebook draws it here with the host NumPy RNG; a test
        injects the reference's)."""
        if eps is None:
            eps = Tensor(np.random.normal(0, 1, size=mu.shape).astype(np.float32), device=device, requires_grad=False)
        return nnet.reparameterize(mu, logvar, eps)

    def forward(self, x, eps=None):
        x = self.encoder(x)
        mu = self.mu_encoder(x)
        logvar = self.logvar_encoder(x)
        z = self.reparameterize(mu, logvar, eps)
        return self.decoder(z), mu, logvar

    def loss_function(self, x, x_recon, mu, logvar):
        BCE = self.loss_fn(x_recon, x)
        KLD = nnet.gaussian_kld(mu, logvar)
        return BCE + KLD

    def train_step(self, in_x, out_x, optimizer, eps=None):
        x_recon, mu, logvar = self.forward(in_x, eps)
        loss = self.loss_function(out_x, x_recon, mu, logvar)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss

    def encode(self, x):
        x = self.encoder(x)
        mu = self.mu_encoder(x)
        logvar = self.logvar_encoder(x)
        return self.reparameterize(mu, logvar)

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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    np.random.seed(args.seed)                                  # initial weights and eps come from the global NumPy RNG, as in the notebook
    rng = np.random.default_rng(args.seed)
    vae = VAE(cfg["input_size"], cfg["latent_size"], cfg["hidden"]).to(device)
    optimizer = Adam(vae.parameters(), lr=0.0005)
    vae.train()
    t0 = None
    for step in range(args.steps):
        if step == min(5, args.steps - 1):
            torch.cuda.synchronize()
            t0, s0 = time.perf_counter(), step
        batch = synthetic_images(rng, cfg["batch"], cfg["input_size"])
        in_x = Tensor(batch, device=device, requires_grad=False)
        out_x = Tensor(batch, device=device, requires_grad=False)
        loss = vae.train_step(in_x, out_x, optimizer)
        if step % 20 == 0 or step == args.steps - 1:
            print(f"step {step:5d}  loss {loss.item():.7f}")
    torch.cuda.synchronize()
    if t0 is not None and args.steps - s0 > 0:
        print(f"{(args.steps - s0) / (time.perf_counter() - t0):.1f} steps/s (eager, {args.config})")


if __name__ == "__main__":
    main()
