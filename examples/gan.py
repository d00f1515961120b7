"""MLP GAN on the HIP path -- the generator, the discriminator and the three-phase training step of the reference's
examples/gan.ipynb (cells 2-3): Linear / LeakyReLU / BatchNorm1d / Dropout / Tanh against Linear / LeakyReLU / Sigmoid, MSELoss,
Adam(lr 0.001, betas (0.5, 0.999)) for each.

    python examples/gan.py --config notebook --steps 200      # noise 100, hidden 256 / 512, 784 pixels, batch 100
    python examples/gan.py --config tiny --steps 20           # the size of tests/golden/gan_tiny.npz

trains on synthetic images (a bright blob on noise, scaled to [-1, 1] as the notebook scales MNIST) and prints the G and D losses
as the notebook computes them, and steps/s.  The step runs eagerly."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip  # noqa: E402,F401
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip import Tensor  # noqa: E402
from neunet_hip.optim import Adam  # noqa: E402

CONFIGS = {"notebook": dict(noise=100, g_hidden=(256, 512), pixels=784, d_hidden=(128, 64), batch=100),
           "tiny": dict(noise=16, g_hidden=(32, 48), pixels=64, d_hidden=(24, 12), batch=12)}


def make_generator(noise, g_hidden, pixels, **_):
    h1, h2 = g_hidden
    return nn.Sequential(nn.Linear(noise, h1), nn.LeakyReLU(), nn.BatchNorm1d(h1), nn.Linear(h1, h2), nn.Dropout(0.2),
                         nn.BatchNorm1d(h2), nn.LeakyReLU(), nn.Linear(h2, pixels), nn.Tanh()).to("cuda")


def make_discriminator(pixels, d_hidden, **_):
    h1, h2 = d_hidden
    return nn.Sequential(nn.Linear(pixels, h1), nn.LeakyReLU(), nn.Linear(h1, h2), nn.LeakyReLU(), nn.Linear(h2, 1),
                         nn.Sigmoid()).to("cuda")


def run_generator(generator, noise, dropout_mask=None):
    """generator(noise); dropout_mask (a device array of the Dropout's input shape, values 0 or 1 / (1 - p)) replaces the mask the
    Dropout would draw -- the parity test injects the reference's."""
    x = noise
    for m in generator.modules:
        x = m.forward(x, mask=dropout_mask) if dropout_mask is not None and isinstance(m, nn.Dropout) else m(x)
    return x


def _const(value, rows):
    return Tensor(np.full((rows, 1), value, np.float32), device="cuda", requires_grad=False)


def train_step(generator, discriminator, g_opt, d_opt, loss_fn, real, noise_d, noise_g, masks=(None, None)):
    """The notebook's step (cell 3), in its order:
        1. d_opt.zero_grad(); real -> loss against ones -> backward -> d_opt.step()
        2. fake = G(noise_d) -> loss against zeros -> backward WITHOUT a zero_grad in between (the discriminator's gradients
           accumulate over phases 1 and 2, and the gradient flows on into the generator) -> d_opt.step()
        3. g_opt.zero_grad(); fake = G(noise_g) -> loss against ones -> backward -> g_opt.step()
    Returns the three losses and the predictions the notebook's printed G / D losses are computed from."""
    rows = real.shape[0]
    d_opt.zero_grad()
    real_pred = discriminator(real)
    real_loss = loss_fn(real_pred, _const(1.0, rows))
    real_loss.backward()
    d_opt.step()

    fake_pred = discriminator(run_generator(generator, noise_d, masks[0]))
    fake_loss = loss_fn(fake_pred, _const(0.0, noise_d.shape[0]))
    fake_loss.backward()
    d_opt.step()

    g_opt.zero_grad()
    fake_pred_g = discriminator(run_generator(generator, noise_g, masks[1]))
    g_loss = loss_fn(fake_pred_g, _const(1.0, noise_g.shape[0]))
    g_loss.backward()
    g_opt.step()
    return real_loss, fake_loss, g_loss, real_pred, fake_pred_g


def printed_losses(real_pred, fake_pred):
    """The notebook's progress line: G loss = -mean log D(G(z)), D loss = -mean log D(x) - mean log(1 - D(G(z)))."""
    rp, fp = real_pred.numpy().astype(np.float64), fake_pred.numpy().astype(np.float64)
    return float(-np.log(fp).mean()), float(-np.log(rp).mean() - np.log(1 - fp).mean())


def synthetic_images(rng, batch, pixels):
    side = int(round(pixels ** 0.5))
    x = rng.uniform(0.0, 0.2, (batch, side, side))
    for i in range(batch):
        r, c = rng.integers(0, max(side - side // 3, 1), 2)
        x[i, r:r + side // 3 + 1, c:c + side // 3 + 1] += 0.8
    return (x.reshape(batch, -1)[:, :pixels] * 2 - 1).astype(np.float32)


def main():
    import argparse
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="notebook")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    np.random.seed(args.seed)                                  # the layers draw their initial weights from the global NumPy RNG
    rng = np.random.default_rng(args.seed)
    generator, discriminator = make_generator(**cfg), make_discriminator(**cfg)
    g_opt = Adam(generator.parameters(), lr=0.001, betas=(0.5, 0.999))
    d_opt = Adam(discriminator.parameters(), lr=0.001, betas=(0.5, 0.999))
    loss_fn = nn.MSELoss()
    generator.train()
    discriminator.train()
    t0 = None
    for step in range(args.steps):
        if step == min(5, args.steps - 1):                     # steps/s without the first launches
            torch.cuda.synchronize()
            t0, s0 = time.perf_counter(), step
        real = Tensor(synthetic_images(rng, cfg["batch"], cfg["pixels"]), device="cuda", requires_grad=False)
        nd, ng = (Tensor(rng.standard_normal((cfg["batch"], cfg["noise"])).astype(np.float32), device="cuda", requires_grad=False)
                  for _ in range(2))
        out = train_step(generator, discriminator, g_opt, d_opt, loss_fn, real, nd, ng)
        if step % 20 == 0 or step == args.steps - 1:
            g_loss, d_loss = printed_losses(out[3], out[4])
            print(f"step {step:5d}  G loss {g_loss:.7f}  D loss {d_loss:.7f}")
    torch.cuda.synchronize()
    if t0 is not None and args.steps - s0 > 0:
        print(f"{(args.steps - s0) / (time.perf_counter() - t0):.1f} steps/s (eager, {args.config})")


if __name__ == "__main__":
    main()
