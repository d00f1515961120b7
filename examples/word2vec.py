"""Word embeddings on the HIP path -- the two models and the training loop of the reference's examples/word2vec.ipynb: a CBOW model
(four context words -> the word between them) and a skip-gram model (a word -> its four context words) over Shakespeare's Sonnet 2,
Embedding -> Linear -> ReLU -> Linear -> Softmax(axis=1) -> .log() -> NLLLoss, one (context, target) pair per step, Adam(lr 0.001),
int16 ids.

    python examples/word2vec.py --model both                      # 50 epochs of each, the notebook's head
    python examples/word2vec.py --model cbow --head logsoftmax    # nn.LogSoftmax instead of Softmax + log

prints the summed loss per epoch, steps/s and the embedding of "beauty".  --head softmax-log is the notebook's forward literally
(`self.softmax(out).log()`, 19 launches per step); --head logsoftmax puts nn.LogSoftmax there, and NLLLoss(LogSoftmax(x)) runs its
backward as ONE pass over the log-probabilities (nnhipLogSoftmaxNLLBackward, 16 launches per step).

One deviation from the notebook: the vocabulary is sorted(set(words)).  The notebook enumerates a `set`, whose order changes with the
hash seed from process to process."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip as nnet  # noqa: E402
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip.optim import Adam  # noqa: E402

CONTEXT_SIZE = 2  # 2 words to the left, 2 to the right
EMBEDDING_DIM = 10
HEADS = ("softmax-log", "logsoftmax")
# Shakespeare, Sonnet 2
SONNET = """When forty winters shall besiege thy brow,
And dig deep trenches in thy beauty's field,
Thy youth's proud livery so gazed on now,
Will be a totter'd weed of small worth held:
Then being asked, where all thy beauty lies,
Where all the treasure of thy lusty days;
To say, within thine own deep sunken eyes,
Were an all-eating shame, and thriftless praise.
How much more praise deserv'd thy beauty's use,
If thou couldst answer 'This fair child of mine
Shall sum my count, and make my old excuse,'
Proving his beauty by succession thine!
This were to be new made when thou art old,
And see thy blood warm when thou feel'st it cold.""".split()


def make_pairs(words, context_size=CONTEXT_SIZE):
    """(vocabulary, [(context ids, target id)]): for every position the `context_size` words before it (nearest first; the first
    positions wrap around to the end of the text, as the notebook's negative indices do) and after it."""
    vocab = sorted(set(words))
    ix = {w: i for i, w in enumerate(vocab)}
    pairs = [([ix[words[i - j - 1]] for j in range(context_size)] + [ix[words[i + j + 1]] for j in range(context_size)], ix[words[i]])
             for i in range(len(words) - context_size)]
    return vocab, pairs


class CBOWModeler(nn.Module):
    """The notebook's class: same attribute names.  hidden = 128 is the notebook's width; head = "logsoftmax" puts nn.LogSoftmax where
    the notebook has `self.softmax(out).log()`."""

    def __init__(self, vocab_size, embedding_dim, context_size, hidden=128, head="softmax-log"):
        super().__init__()
        self.vocab_size = vocab_size
        self.embedding_dim = embedding_dim
        self.context_size = context_size

        self.embeddings = nn.Embedding(vocab_size, embedding_dim)
        self.linear1 = nn.Linear(2 * context_size * embedding_dim, hidden)
        self.linear2 = nn.Linear(hidden, vocab_size)
        self.relu = nn.ReLU()
        self.softmax = nn.Softmax(axis=1)
        self.log_softmax = nn.LogSoftmax(axis=1)
        if head not in HEADS:
            raise ValueError(f"head must be one of {HEADS}")
        self.head = head

    def forward(self, inputs):
        embeds = self.embeddings(inputs).reshape((1, -1))
        out = self.relu(self.linear1(embeds))
        out = self.linear2(out)
        if self.head == "logsoftmax":
            return self.log_softmax(out)
        log_probs = self.softmax(out).log()
        return log_probs


class SkipGramModeler(nn.Module):
    """The notebook's class: same attribute names; one row of log-probabilities per context position."""

    def __init__(self, vocab_size, embedding_dim, context_size, hidden=128, head="softmax-log"):
        super().__init__()
        self.vocab_size = vocab_size
        self.embedding_dim = embedding_dim
        self.context_size = context_size

        self.embeddings = nn.Embedding(vocab_size, embedding_dim)
        self.linear1 = nn.Linear(embedding_dim, hidden)
        self.linear2 = nn.Linear(hidden, 2 * context_size * vocab_size)
        self.relu = nn.ReLU()
        self.softmax = nn.Softmax(axis=1)
        self.log_softmax = nn.LogSoftmax(axis=1)
        if head not in HEADS:
            raise ValueError(f"head must be one of {HEADS}")
        self.head = head

    def forward(self, inputs):
        embeds = self.embeddings(inputs).reshape((1, -1))
        out = self.relu(self.linear1(embeds))
        out = self.linear2(out).reshape(2 * self.context_size, -1)
        if self.head == "logsoftmax":
            return self.log_softmax(out)
        log_probs = self.softmax(out).log()
        return log_probs


def pair_tensors(kind, context, target):
    """(input ids, labels) of one pair as int16 device tensors: CBOW reads the context and predicts the target, skip-gram the reverse."""
    ids, labels = (context, [target]) if kind == "cbow" else ([target], context)
    return (nnet.tensor(ids, dtype=np.int16, requires_grad=False, device="cuda"),
            nnet.tensor(labels, dtype=np.int16, requires_grad=False, device="cuda"))


def train(kind, epochs, head="softmax-log", words=SONNET, quiet=False):
    """The notebook's loop.  Returns (model, vocabulary, the summed loss of every epoch)."""
    vocab, pairs = make_pairs(words)
    model = (CBOWModeler if kind == "cbow" else SkipGramModeler)(len(vocab), EMBEDDING_DIM, CONTEXT_SIZE, head=head).to("cuda")
    loss_function = nn.NLLLoss()
    optimizer = Adam(model.parameters(), lr=0.001)
    data = [pair_tensors(kind, c, t) for c, t in pairs]
    totals = []
    t0 = time.perf_counter()
    for epoch in range(epochs):
        losses = []
        for ids, labels in data:
            optimizer.zero_grad()
            log_probs = model(ids)
            loss = loss_function(log_probs, labels)
            loss.backward()
            optimizer.step()
            losses.append(loss.data)
        totals.append(float(sum(l.item() for l in losses)))      # one host read per loss, after the epoch's last launch
        if not quiet:
            print(f"{kind} epoch {epoch + 1:3d}  loss: {totals[-1]:.7f}")
    dt = time.perf_counter() - t0
    if not quiet:
        print(f"{kind}: {epochs * len(data) / dt:.1f} steps/s ({head} head, {len(data)} pairs per epoch, vocabulary {len(vocab)})")
    return model, vocab, totals


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("cbow", "skipgram", "both"), default="both")
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--head", choices=HEADS, default="softmax-log")
    a = ap.parse_args(argv)
    np.random.seed(0)        # the layers draw their initial weights from the global generator
    results = {}
    for kind in (("cbow", "skipgram") if a.model == "both" else (a.model,)):
        model, vocab, totals = train(kind, a.epochs, a.head)
        print(f'Embedding of the word "beauty":\n{model.embeddings.weight.numpy()[vocab.index("beauty")]}')
        results[kind] = totals
    return results


if __name__ == "__main__":
    main()
