"""Step-decoding captioner over the pycaffe-style API (the counterpart of
the reference's examples/coco/captioner.py).

The LSTM deploy net has T = 1: one forward per token, N caption streams in
parallel, `cont_sentence` 0 on the first token and 1 afterwards.  Its
recurrent layers carry h/c between forwards (pycaffe.Net's default), so a
caption of L tokens costs L single-token forwards, and the image net runs
once per image.

    cap = Captioner("lrcn.caffemodel", "image.deploy.prototxt",
                    "lrcn_word_to_preds.deploy.prototxt", vocab, device)
    desc = cap.compute_descriptors(images, "fc8")
    cap.set_caption_batch_size(1)
    tokens, probs = cap.sample_captions(desc[0])
    print(cap.sentence(tokens[0]))
"""

from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import pycaffe
from .vocab import EOS, Vocab

EOS_ID = 0


def _load_vocab(vocab) -> List[str]:
    if isinstance(vocab, Vocab):
        return list(vocab.words)
    if isinstance(vocab, str):
        if vocab.endswith(".json"):
            return list(Vocab.load(vocab).words)
        # one word per line, the end-of-sentence token implied at id 0
        with open(vocab) as fh:
            return [EOS] + [ln.strip() for ln in fh if ln.strip()]
    return list(vocab)


class Captioner:
    def __init__(self, weights: Optional[str], image_net_proto: Optional[str],
                 lstm_net_proto: str, vocab,
                 device: Optional[torch.device] = None, *, seed: int = 0):
        self.device = device or torch.device("cpu")
        self.image_net = None
        if image_net_proto:
            self.image_net = pycaffe.Net(image_net_proto, weights,
                                         pycaffe.TEST, device=self.device)
        self.lstm_net = pycaffe.Net(lstm_net_proto, weights, pycaffe.TEST,
                                    device=self.device,
                                    stateful_recurrent=True)
        self.vocab = _load_vocab(vocab)
        self.generator = torch.Generator().manual_seed(seed)
        net = self.lstm_net._net
        for name in ("cont_sentence", "input_sentence", "image_features"):
            if name not in net.blob_map:
                raise ValueError(f"LSTM net has no input blob {name!r}")

    # ------------------------------------------------------------ image net
    def compute_descriptors(self, images, output_name: str = "fc8"):
        """Run the image net over preprocessed images ([C,H,W] arrays or one
        [B,C,H,W] batch) and return blob `output_name` as [B, ...] float32."""
        if self.image_net is None:
            raise RuntimeError("Captioner was built without an image net")
        batch = np.stack([np.asarray(im, dtype=np.float32) for im in images]) \
            if not (isinstance(images, np.ndarray) and images.ndim == 4) \
            else images.astype(np.float32)
        self.image_net.forward(data=batch)
        return self.image_net.blobs[output_name].data.reshape(
            batch.shape[0], -1)

    # ------------------------------------------------------------- LSTM net
    @property
    def caption_batch_size(self) -> int:
        return self.lstm_net.blobs["cont_sentence"].shape[1]

    def set_caption_batch_size(self, n: int) -> None:
        blobs = self.lstm_net.blobs
        feat = blobs["image_features"].shape
        blobs["cont_sentence"].reshape(1, n)
        blobs["input_sentence"].reshape(1, n)
        blobs["image_features"].reshape(n, *feat[1:])
        self.lstm_net.reshape()
        self.lstm_net.reset_recurrent_state()

    def sample_captions(self, descriptor, temp: float = float("inf"),
                        max_length: int = 50,
                        prob_output_name: str = "probs",
                        pred_output_name: str = "predict"):
        """Decode one caption per stream, a token per forward.

        descriptor: [F] (repeated over the streams) or [N, F].
        temp = inf takes the arg-max (greedy); a finite temp samples from
        softmax(temp * predict), temp being the reference's inverse
        temperature, with this object's seeded generator.
        A stream stops at EOS (token 0), which closes its token list.
        Returns (tokens, probs): per stream the token ids and the
        probability the net gave each."""
        net = self.lstm_net._net
        n = self.caption_batch_size
        dev, dt = net.device, net.dtype
        feats = torch.as_tensor(np.asarray(descriptor, dtype=np.float32))
        if feats.dim() == 1:
            feats = feats.unsqueeze(0).expand(n, -1)
        if feats.shape[0] != n:
            raise ValueError(f"{feats.shape[0]} descriptors for {n} caption "
                             "streams; call set_caption_batch_size first")
        net.blob_by_name("image_features").data = \
            feats.contiguous().to(dev, dt)
        tokens: List[List[int]] = [[] for _ in range(n)]
        probs: List[List[float]] = [[] for _ in range(n)]
        done = [False] * n
        word = torch.zeros(1, n)
        greedy = math.isinf(temp)
        for step in range(max_length):
            net.blob_by_name("cont_sentence").data = torch.full(
                (1, n), 0.0 if step == 0 else 1.0).to(dev, dt)
            # token ids stay fp32: bf16 cannot hold a 4-digit index
            net.blob_by_name("input_sentence").data = word.to(dev)
            net.forward(read_loss=False)
            p = net.blob_by_name(prob_output_name).data[0].float()
            if greedy:
                nxt = p.argmax(dim=1)
            else:
                logits = net.blob_by_name(pred_output_name).data[0].float()
                q = torch.softmax(logits * float(temp), dim=1).cpu()
                nxt = torch.multinomial(q, 1, generator=self.generator)[:, 0]
                nxt = nxt.to(p.device)
            pn = p.gather(1, nxt.reshape(n, 1))[:, 0].tolist()
            nxt_l = nxt.tolist()
            for i in range(n):
                if done[i]:
                    continue
                tokens[i].append(int(nxt_l[i]))
                probs[i].append(float(pn[i]))
                done[i] = nxt_l[i] == EOS_ID
            if all(done):
                break
            word = torch.tensor([nxt_l], dtype=torch.float32)
        return tokens, probs

    def sentence(self, indices: Sequence[int]) -> str:
        words = []
        for i in indices:
            if i == EOS_ID:
                break
            words.append(self.vocab[i] if 0 <= i < len(self.vocab)
                         else str(i))
        return " ".join(words)
