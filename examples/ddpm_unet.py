"""DDPM U-Net on the HIP path -- the module graph of the reference's examples/ddpm.ipynb (cells 5-7: ResBlock, SimpleUNet) and
one training step of its Diffusion.forward (cell 4: noise an image to a random timestep with the linear beta schedule, predict
the noise, MSE, Adam lr 2e-4).  The module tree and the attribute order are the notebook's, so parameters() lines up with a
model the reference built.  The sinusoidal time embedding has no parameters and is computed on the host.

    python examples/ddpm_unet.py --config utkface --batch 5 --steps 10     # 3 x 32 x 32, channels 128..1024 (notebook cell 8)
    python examples/ddpm_unet.py --config mnist --batch 16 --steps 10      # 1 x 28 x 28, channels 32..128

trains on seeded synthetic images and prints the loss per step and steps/s."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip  # noqa: E402
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip import Tensor  # noqa: E402

TIME_EMB_DIM = 32
CONFIGS = {"utkface": dict(image_channels=3, image_size=32, down_channels=(128, 256, 512, 1024)),
           "mnist": dict(image_channels=1, image_size=28, down_channels=(32, 64, 128))}


class ResBlock(nn.Module):
    def __init__(self, input_channels, output_channels, time_emb_dim, up=False):
        super().__init__()
        self.time_embedding = nn.Linear(time_emb_dim, output_channels)
        self.input_channels = input_channels
        self.output_channels = output_channels
        if up:
            self.conv1 = nn.Conv2d(2 * input_channels, output_channels, kernel_size=(3, 3), padding=(1, 1))
            self.transform = nn.ConvTranspose2d(output_channels, output_channels, kernel_size=(4, 4), stride=(2, 2), padding=(1, 1))
        else:
            self.conv1 = nn.Conv2d(input_channels, output_channels, kernel_size=(3, 3), padding=(1, 1))
            self.transform = nn.Conv2d(output_channels, output_channels, kernel_size=(4, 4), stride=(2, 2), padding=(1, 1))
        self.conv2 = nn.Conv2d(output_channels, output_channels, kernel_size=(3, 3), padding=(1, 1))
        self.relu1 = nn.LeakyReLU(alpha=0.01)
        self.relu2 = nn.LeakyReLU(alpha=0.01)
        self.relu3 = nn.LeakyReLU(alpha=0.01)
        self.bnorm1 = nn.BatchNorm2d(output_channels, momentum=0.1, eps=1e-5)
        self.bnorm2 = nn.BatchNorm2d(output_channels, momentum=0.1, eps=1e-5)

    def forward(self, x, t):
        h = self.bnorm1(self.relu1(self.conv1(x)))
        time_emb = self.relu2(self.time_embedding(t))
        h = neunet_hip.add_channel_bias(h, time_emb)
        h = self.bnorm2(self.relu3(self.conv2(h)))
        return self.transform(h)


def time_encoding(t, d_model=TIME_EMB_DIM):
    """What the notebook's PositionalEncoding (cell 6) makes of SimpleUNet's t[:, None, None]: the sinusoid table's row b (the
    position in the BATCH, as the notebook indexes it) plus the scalar t_b, -> [B, d_model] float32."""
    t = np.asarray(t, dtype=np.float32)
    pe = np.zeros((len(t), d_model))
    position = np.arange(len(t))[:, None]
    div_term = np.exp(np.arange(0, d_model, 2) * (-np.log(10000.0) / d_model))
    pe[:, 0::2] = np.sin(position * div_term)
    pe[:, 1::2] = np.cos(position * div_term)
    return t[:, None] + pe.astype(np.float32)


class SimpleUNet(nn.Module):
    def __init__(self, image_channels, image_size, down_channels=(32, 64, 128, 256, 512), up_channels=None):
        super().__init__()
        up_channels = tuple(down_channels[::-1]) if up_channels is None else up_channels
        noise_channels = image_channels
        # (the notebook's Sequential starts with the parameter-free PositionalEncoding: time_encoding() above)
        self.time_embedding = nn.Sequential(nn.Linear(TIME_EMB_DIM, TIME_EMB_DIM), nn.LeakyReLU())
        if image_size & (image_size - 1) != 0:
            self.input_conv = nn.ConvTranspose2d(image_channels, down_channels[0], kernel_size=(5, 5))
            self.output_conv = nn.Conv2d(up_channels[-1], noise_channels, kernel_size=(5, 5))
        else:
            self.input_conv = nn.Conv2d(image_channels, down_channels[0], kernel_size=(3, 3), padding=(1, 1))
            self.output_conv = nn.ConvTranspose2d(up_channels[-1], noise_channels, kernel_size=(3, 3), padding=(1, 1))
        self.down_layers = nn.ModuleList([ResBlock(down_channels[i], down_channels[i + 1], TIME_EMB_DIM)
                                          for i in range(len(down_channels) - 1)])
        self.up_layers = nn.ModuleList([ResBlock(up_channels[i], up_channels[i + 1], TIME_EMB_DIM, up=True)
                                        for i in range(len(up_channels) - 1)])

    def forward(self, x, t):
        """x: device Tensor [B, C, S, S]; t: host array of timestep fractions in [0, 1), one per image."""
        t = self.time_embedding(Tensor(time_encoding(t), requires_grad=False, device=x.device))
        x = self.input_conv(x)
        residual_inputs = []
        for down_layer in self.down_layers:
            x = down_layer(x, t)
            residual_inputs.append(x)
        for up_layer in self.up_layers:
            x = up_layer(neunet_hip.concatenate(x, residual_inputs.pop(), axis=1), t)
        return self.output_conv(x)


class Diffusion:
    """The training half of the notebook's Diffusion (cell 4): the linear beta schedule and Algorithm 1 of arXiv:2006.11239."""

    def __init__(self, model, timesteps=300, beta_start=0.0001, beta_end=0.02, lr=2e-4):
        from neunet_hip.optim import Adam
        self.model, self.timesteps = model, timesteps
        betas = np.linspace(beta_start, beta_end, timesteps, dtype=np.float32)
        alphas_cumprod = np.cumprod(1 - betas, axis=0, dtype=np.float32)
        self.sqrt_alphas_cumprod = np.sqrt(alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1 - alphas_cumprod)
        self.criterion = nn.MSELoss()
        self.optimizer = Adam(model.parameters(), lr=lr)

    def noised(self, x0, t, noise):
        return (self.sqrt_alphas_cumprod[t, None, None, None] * x0
                + self.sqrt_one_minus_alphas_cumprod[t, None, None, None] * noise).astype(np.float32)

    def loss(self, x0, t, noise):
        """x0, noise: host [B, C, S, S]; t: host int timesteps -> (loss Tensor, predicted noise Tensor)"""
        x_t = Tensor(self.noised(x0, t, noise), requires_grad=False, device="cuda")
        pred = self.model(x_t, t / self.timesteps)
        return self.criterion(pred, Tensor(noise, requires_grad=False, device="cuda")), pred

    def train_step(self, x0, t, noise):
        self.optimizer.zero_grad()
        loss, _ = self.loss(x0, t, noise)
        loss.backward()
        self.optimizer.step()
        return loss


def main():
    import argparse

    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="utkface")
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    np.random.seed(0)
    rng = np.random.default_rng(0)
    diffusion = Diffusion(SimpleUNet(**cfg).to("cuda"))
    C, S = cfg["image_channels"], cfg["image_size"]
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32) / S
    t0 = None
    for step in range(args.steps):
        # synthetic images: a smooth blob at a random place per image, in [-1, 1]
        cy, cx = rng.uniform(0.2, 0.8, (2, args.batch, 1, 1, 1)).astype(np.float32)
        x0 = (2 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) * 20) - 1) * np.ones((1, C, 1, 1), np.float32)
        t = rng.integers(1, diffusion.timesteps, (args.batch,)).astype(np.int32)
        noise = rng.standard_normal(x0.shape).astype(np.float32)
        loss = diffusion.train_step(x0.astype(np.float32), t, noise)
        print(f"step {step:4d}  loss {loss.item():.4f}", flush=True)
        if step == 0:                                   # the first step pays for workspace growth and kernel loading
            torch.cuda.synchronize()
            t0 = time.perf_counter()
    torch.cuda.synchronize()
    if args.steps > 1:
        print(f"{(args.steps - 1) / (time.perf_counter() - t0):.2f} steps/s ({args.config}, batch {args.batch}, eager, first step excluded)")


if __name__ == "__main__":
    main()
