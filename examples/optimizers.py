"""Optimizer trajectories on the HIP path -- the reference's examples/optimizers_visualization.ipynb: every optimizer of
neunet_hip.optim descends one of the notebook's six test surfaces (Himmelblau by default) from the notebook's starting point
(0, -7) at the notebook's learning rate 0.01, one two-element parameter on the device, one kernel launch per step.

    python examples/optimizers.py                                        # 1000 iterations, the notebook's run
    python examples/optimizers.py --function rosenbrock --iterations 200 --save trajectories.npz

prints where each optimizer ends and the function value there; --save writes every trajectory ((iterations + 1, 2) points per
optimizer, plus its function values) to an .npz for plotting elsewhere -- no matplotlib here.

The notebook's eight optimizers plus AdamW.  The surface's gradient at the current point comes from torch's autograd on the
device (neunet_hip's Tensor has no elementwise arithmetic to differentiate through); the update is the library's."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip  # noqa: E402,F401
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip import Tensor  # noqa: E402
from neunet_hip.optim import SGD, Adadelta, Adagrad, Adam, Adamax, AdamW, Momentum, NAdam, RMSprop  # noqa: E402


def rosenbrock(x, y):
    return (1 - x) ** 2 + 100 * (y - x**2) ** 2


def himmelblau(x, y):
    return (x**2 + y - 11) ** 2 + (x + y**2 - 7) ** 2


def matyas(x, y):
    return 0.26 * (x**2 + y**2) - 0.48 * x * y


def beale(x, y):
    return (1.5 - x + x * y) ** 2 + (2.25 - x + x * y**2) ** 2 + (2.625 - x + x * y**3) ** 2


def booth(x, y):
    return (x + 2 * y - 7) ** 2 + (2 * x + y - 5) ** 2


def goldstein_price(x, y):
    return (1 + (x + y + 1) ** 2 * (19 - 14 * x + 3 * x**2 - 14 * y + 6 * x * y + 3 * y**2)) * (
        30 + (2 * x - 3 * y) ** 2 * (18 - 32 * x + 12 * x**2 + 48 * y - 36 * x * y + 27 * y**2)
    )


FUNCTIONS = {f.__name__: f for f in (rosenbrock, himmelblau, matyas, beale, booth, goldstein_price)}
OPTIMIZERS = [Adam, SGD, RMSprop, NAdam, Momentum, Adagrad, Adadelta, Adamax, AdamW]      # the notebook's order, then AdamW
STARTING_POINT = (-0.0, -7.0)       # (x, y)
LEARNING_RATE = 0.01


def gradient_descent(starting_point, optimizer, num_iterations, function, learning_rate):
    """The notebook's gradient_descent: the (num_iterations + 1, 2) points visited, the starting point first."""
    import torch
    point = nn.Parameter(Tensor(np.asarray(starting_point, np.float32), device="cuda"))
    optimizer = optimizer(lr=learning_rate, params=[point])
    points = torch.empty((num_iterations + 1, 2), dtype=torch.float32, device="cuda")
    points[0] = point.data
    for it in range(num_iterations):
        optimizer.zero_grad()
        at = point.data.detach().clone().requires_grad_(True)
        function(at[0], at[1]).backward()
        point.grad = at.grad
        optimizer.step()
        points[it + 1] = point.data
    return points.cpu().numpy()


def run(function=himmelblau, num_iterations=1000, starting_point=STARTING_POINT, learning_rate=LEARNING_RATE, optimizers=OPTIMIZERS):
    """{optimizer name: (points (iterations + 1, 2), function values (iterations + 1,) in float64)}"""
    out = {}
    for optimizer in optimizers:
        points = gradient_descent(starting_point, optimizer, num_iterations, function, learning_rate)
        p64 = points.astype(np.float64)
        out[optimizer.__name__] = (points, function(p64[:, 0], p64[:, 1]))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--function", choices=sorted(FUNCTIONS), default="himmelblau")
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=LEARNING_RATE)
    ap.add_argument("--save", default=None, help="write the trajectories to this .npz")
    a = ap.parse_args(argv)
    function = FUNCTIONS[a.function]
    results = run(function, a.iterations, STARTING_POINT, a.lr)
    print(f"{a.function} from {STARTING_POINT}, lr {a.lr}, {a.iterations} iterations")
    for name, (points, values) in results.items():
        print(f"{name:9s} f {values[0]:12.4f} -> {values[-1]:12.6f} at ({points[-1, 0]: .5f}, {points[-1, 1]: .5f})")
    if a.save:
        arrays = {}
        for name, (points, values) in results.items():
            arrays[f"{name}_points"], arrays[f"{name}_values"] = points, values
        np.savez_compressed(a.save, **arrays)
        print("saved", a.save)
    return results


if __name__ == "__main__":
    main()
