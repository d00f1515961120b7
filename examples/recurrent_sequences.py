"""Sentence sentiment classifier on the HIP path -- the model and training loop of the reference's
examples/recurrent_sequences_classifier.ipynb (cells 2-7):

    Embedding(40, 10) -> Bidirectional(GRU(10, 50, all), "sum") -> Bidirectional(RNN(50, 50, all)) -> Bidirectional(GRU(50, 50, last))
    -> Linear(50, 1) -> Sigmoid, MSELoss, Adam(lr 0.001), one sentence (batch 1, T = 5) per step.

`python examples/recurrent_sequences.py --epochs 100` trains on the notebook's ten sentences and prints the final loss and the
accuracy; --graphed replays every step from a captured hipGraph (neunet_hip.graph.GraphedTrainStep).  Each Bidirectional layer is one
projection per direction, ONE recurrence launch for both directions and one merge launch, whatever T is.

Differences from the notebook: the vocabulary is built from the SORTED word set (the notebook iterates a Python set, whose order
changes from run to run); a sentence that already has the maximal length is kept as it is (the notebook's padding loop assigns
`padded_line` only under `if len(...) < max_length`, so it appends the previous sentence again in its place); the label is reshaped
to the prediction's (1, 1, 1) (HIPMSELoss wants equal shapes; the reference broadcasts (1,) against (1, 1, 1) to the same value)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip  # noqa: E402,F401
import neunet_hip.nn as nn  # noqa: E402

DOCUMENT = ["Nice Clothes!", "Very good shop for clothes", "Amazing clothes", "Clothes are good", "Superb!", "Very bad", "Poor quality",
            "not good", "clothes fitting bad", "Shop not good"]
LABELS = [1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
VOCAB_SIZE = 40
CHARS2REMOVE = '!"#$%&()*+,-./:;<=>?@[\\]^_`{|}~\t\n'


def encode_document(document=DOCUMENT, vocab_size=VOCAB_SIZE):
    """Cell 3: strip punctuation, lower-case, give every word a distinct random id in 1 .. vocab_size - 1 (drawn from the global NumPy
    generator), pad with 0 to the longest sentence.  Returns (int32 [sentences, max_length], vocabulary)."""
    import numpy as np
    filtered = ["".join(c for c in line if c not in CHARS2REMOVE) for line in document]
    words = sorted({w.lower() for line in filtered for w in line.split()})
    ids = np.random.choice(range(1, vocab_size), len(words), replace=False)
    vocab = dict(zip(words, (int(i) for i in ids)))
    encoded = [[vocab[w.lower()] for w in line.split()] for line in filtered]
    max_length = max(len(e) for e in encoded)
    return np.array([e + [0] * (max_length - len(e)) for e in encoded], np.int32), vocab


class SequenceClassifier(nn.Module):
    """Cell 4's nn.Sequential, with names; parameters() walks the same order."""

    def __init__(self, vocab_size=VOCAB_SIZE, embed=10, hidden=50):
        super().__init__()
        self.embedding = nn.Embedding(vocab_size, embed)
        self.bi1 = nn.Bidirectional(nn.GRU(embed, hidden, return_sequences=True), merge_mode="sum")
        self.bi2 = nn.Bidirectional(nn.RNN(hidden, hidden, return_sequences=True, bias=True))
        self.bi3 = nn.Bidirectional(nn.GRU(hidden, hidden, return_sequences=False))
        self.fc = nn.Linear(hidden, 1)
        self.sigmoid = nn.Sigmoid()

    def forward(self, tokens):
        x = self.embedding(tokens)                          # (T,) ids -> (T, embed): a single sequence, batch 1
        x = self.bi3(self.bi2(self.bi1(x)))                 # (1, T, hidden) -> (1, T, hidden) -> (1, 1, hidden)
        return self.sigmoid(self.fc(x))                     # (1, 1, 1)


def main():
    import argparse

    import numpy as np
    import torch
    from neunet_hip import Tensor
    from neunet_hip.optim import Adam
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--graphed", action="store_true", help="replay each step from a captured hipGraph")
    args = ap.parse_args()
    np.random.seed(args.seed)
    docs, _ = encode_document()
    model = SequenceClassifier().to("cuda")
    opt = Adam(model.parameters(), lr=args.lr)
    loss_fn = nn.MSELoss()
    tok = Tensor(docs[0], dtype=np.int32, device="cuda", requires_grad=False)
    lab = Tensor(np.zeros((1, 1, 1), np.float32), device="cuda", requires_grad=False)
    docs_d = torch.from_numpy(docs).cuda()
    labels_d = torch.tensor(LABELS, dtype=torch.float32, device="cuda").reshape(-1, 1, 1, 1)

    def fb():
        loss = loss_fn(model(tok), lab)
        loss.backward()
        return loss

    step_fn = None
    if args.graphed:
        from neunet_hip.distributed import GradBucket
        from neunet_hip.graph import GraphedTrainStep
        step_fn = GraphedTrainStep(fb, opt, GradBucket(model.parameters()), warmup=2)
    loss = None
    for epoch in range(args.epochs):
        for i in range(docs.shape[0]):
            tok.data.copy_(docs_d[i])
            lab.data.copy_(labels_d[i])
            if step_fn is not None:
                loss = step_fn()
            else:
                opt.zero_grad()
                loss = fb()
                opt.step()
        if epoch % 10 == 0 or epoch == args.epochs - 1:
            print(f"epoch {epoch + 1:4d}/{args.epochs}  loss {loss.item():.7f}", flush=True)
    if step_fn is not None:
        step_fn.release()
    correct = 0
    for i in range(docs.shape[0]):
        tok.data.copy_(docs_d[i])
        correct += int(round(float(model(tok).numpy().reshape(-1)[0])) == LABELS[i])
    print(f"final loss {loss.item():.7f}  accuracy {100.0 * correct / docs.shape[0]:.1f} %")


if __name__ == "__main__":
    main()
