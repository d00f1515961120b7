"""Conway's Game of Life learned by a two-layer convolutional net, on the HIP path -- the model, the dataset and the training loop of
the reference's examples/conway.ipynb: GameOfLife (the rule as a fixed 3x3 convolution that counts neighbours), the dataset of all
2^9 = 512 three-by-three neighbourhoods with the rule's answer for each, Net = Conv2d(1, 10, 3) -> neunet_hip.tanh -> Conv2d(10, 1, 1),
one neighbourhood per step, MSE, Adam(lr 0.01) or --optimizer sgd (lr 0.1).

    python examples/conway.py --epochs 20                  # nn.MSELoss
    python examples/conway.py --epochs 20 --loss composed  # ((y_pred - y) ** 2).mean() written with the Tensor operators

prints the mean loss per epoch, steps/s, the number of the 512 cases on which the trained net (rounded at 0.5) disagrees with the
rule, and the number of cells on which it disagrees after --generations steps of the Gosper glider gun on a 64 x 64 torus.  No
matplotlib.  The notebook's `tensor[None, None]` indexing is done in NumPy before the tensor is made (Tensor.__getitem__ is not
provided)."""
import argparse
import itertools
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip as nnet  # noqa: E402
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip.optim import SGD, Adam  # noqa: E402

# the Gosper glider gun in run-length encoding (b dead, o alive, $ end of row; conwaylife.com/wiki/Gosper_glider_gun)
GUN_RLE = "24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o$2o8bo3bob2o4bobo$10bo5bo7bo$11bo3bo$12b2o!"
NEIGHBOURS = np.array([[[[1, 1, 1], [1, 0, 1], [1, 1, 1]]]], np.float32)


def wrap4(grid):
    """[1, 1, H + 2, W + 2]: the grid padded by one cell all round with its opposite edge (a torus)."""
    return np.pad(np.asarray(grid, np.float32), 1, mode="wrap")[None, None]


class GameOfLife(nn.Module):
    """The rule: a cell lives on with 2 or 3 live neighbours and is born with exactly 3; the count is one 3x3 convolution."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(1, 1, 3, padding=0, bias=False)
        self.conv.weight.data.copy_(nnet.Tensor(NEIGHBOURS, device="cuda").data)

    def forward(self, grid):
        grid = np.asarray(grid)
        n = np.rint(self.conv(nnet.Tensor(wrap4(grid), device="cuda", requires_grad=False)).numpy()[0, 0]).astype(int)
        return (n == 3) | ((grid.astype(int) == 1) & (n == 2))


def dataset(game):
    X = np.array([np.array(x).reshape(3, 3) for x in itertools.product([0, 1], repeat=9)])
    return X, np.array([game(x).astype(int) for x in X])


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 10, 3, padding=0)
        self.conv2 = nn.Conv2d(10, 1, 1)

    def forward(self, x):
        return self.conv2(nnet.tanh(self.conv1(x)))

    def predict(self, grid):
        return self.forward(nnet.Tensor(wrap4(grid), device="cuda", requires_grad=False)).numpy()[0, 0]


def make_loss(kind):
    if kind == "module":
        return nn.MSELoss()
    return lambda y_pred, y: ((y_pred - y) ** 2).mean()


def train(model, X, Y, epochs, loss_kind="module", optimizer="adam", seed=0, max_steps=None, log=print):
    """-> per-step losses.  One neighbourhood per step, a fresh permutation per epoch (drawn from default_rng(seed))."""
    opt = Adam(model.parameters(), lr=0.01) if optimizer == "adam" else SGD(model.parameters(), lr=0.1)
    criterion, rng, losses = make_loss(loss_kind), np.random.default_rng(seed), []
    for epoch in range(epochs):
        first = len(losses)
        for i in rng.permutation(len(X)):
            opt.zero_grad()
            x = nnet.Tensor(wrap4(X[i]), device="cuda", requires_grad=False)
            y = nnet.Tensor(np.asarray(Y[i], np.float32)[None, None], device="cuda", requires_grad=False)
            loss = criterion(model(x), y)
            loss.backward()
            opt.step()
            losses.append(loss)
            if max_steps is not None and len(losses) >= max_steps:
                return [l.item() for l in losses]
        losses[first:] = [l.item() for l in losses[first:]]         # one host read per epoch, not per step
        log(f"epoch {epoch + 1}/{epochs}  mean loss {np.mean(losses[first:]):.7f}")
    return losses


def disagreements(model, X, Y):
    """How many of the 512 cases the net (rounded at 0.5) gets wrong."""
    return int(sum(((model.predict(x) > 0.5).astype(int) != y).any() for x, y in zip(X, Y)))


def decode_rle(rle):
    """[(row, column)] of the live cells of a run-length encoded pattern."""
    cells, row, col, count = [], 0, 0, ""
    for ch in rle:
        if ch.isdigit():
            count += ch
            continue
        n, count = int(count or 1), ""
        if ch == "o":
            cells += [(row, col + k) for k in range(n)]
        if ch in "bo":
            col += n
        elif ch == "$":
            row, col = row + n, 0
    return cells


def gun_grid(n=64):
    grid = np.zeros((n, n), np.float32)
    for r, c in decode_rle(GUN_RLE):
        grid[r, c] = 1
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--loss", choices=("module", "composed"), default="module")
    ap.add_argument("--optimizer", choices=("adam", "sgd"), default="adam")
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    np.random.seed(a.seed)
    game, model = GameOfLife(), Net()
    X, Y = dataset(game)
    t0 = time.time()
    losses = train(model, X, Y, a.epochs, a.loss, a.optimizer, a.seed)
    print(f"{len(losses) / (time.time() - t0):.0f} steps/s ({a.loss} loss, {a.optimizer})")
    print(f"cases of 512 the net gets wrong: {disagreements(model, X, Y)}")
    truth = net = gun_grid()
    for _ in range(a.generations):
        truth, net = game(truth).astype(np.float32), (model.predict(net) > 0.5).astype(np.float32)
    print(f"cells that differ from the rule after {a.generations} generations of the glider gun: {int((truth != net).sum())}")


if __name__ == "__main__":
    main()
