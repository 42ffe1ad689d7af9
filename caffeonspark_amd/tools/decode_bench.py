"""Caption-decode benchmark: milliseconds per token of the LRCN
word-to-predictions net (Embed 8801x1000, LSTM 1000, LSTM 1000 with a
1000-wide static input, InnerProduct 8801, Softmax), bf16, seeded random
weights, by three methods:

    python -m caffeonspark_amd.tools.decode_bench

  unrolled  re-run a T=20 build of the net once per token, every LSTM
            starting from zeros (how examples/image_caption.py decodes
            without -lstmNet; the LSTM part only, no image net)
  gemm      stateful T=1 step decode with COS_LSTM_STEP=0: per layer and
            token two or three GEMMs plus the LSTM-unit kernel
  fused     stateful T=1 step decode through the fused step kernel (one
            launch per LSTM layer per token); where N is beyond what the
            kernel serves the layer reports route "gemm" and the row says so

for N = 1, 4, 16, 64 caption streams.  The input tokens are fixed (no
arg-max, no host read-back inside a window): the figures are forward time,
device events around whole net forwards, launch gaps included.  After a
warm-up window per method the three alternate in timed windows.  Next to the
times the tool prints what the shapes imply (weight bytes a token must
read), the end-to-end bytes/s of the fused method against the measured HBM
ceiling, and each layer's share of a fused token, timed layer by layer.
Needs a GPU: without one it fails.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics

import torch

from ..core.net import Net
from ..proto import caffe_pb, text_format

V, E, H, DS, TOKENS = 8801, 1000, 1000, 1000, 20
# measured HBM streaming ceiling of the MI355X, bytes/s
HBM_CEILING = 6.29e12


def net_text(T: int, N: int) -> str:
    return f'''
name: "lrcn_word_to_preds"
input: "cont_sentence" input_shape {{ dim: {T} dim: {N} }}
input: "input_sentence" input_shape {{ dim: {T} dim: {N} }}
input: "image_features" input_shape {{ dim: {N} dim: {DS} }}
layer {{ name: "embedding" type: "Embed" bottom: "input_sentence"
  top: "embedded_input_sentence"
  embed_param {{ input_dim: {V} num_output: {E} bias_term: false }} }}
layer {{ name: "lstm1" type: "LSTM" bottom: "embedded_input_sentence"
  bottom: "cont_sentence" top: "lstm1"
  recurrent_param {{ num_output: {H} }} }}
layer {{ name: "lstm2" type: "LSTM" bottom: "lstm1" bottom: "cont_sentence"
  bottom: "image_features" top: "lstm2"
  recurrent_param {{ num_output: {H} }} }}
layer {{ name: "predict" type: "InnerProduct" bottom: "lstm2" top: "predict"
  inner_product_param {{ axis: 2 num_output: {V} }} }}
layer {{ name: "probs" type: "Softmax" bottom: "predict" top: "probs"
  softmax_param {{ axis: 2 }} }}
'''


def weight_bytes() -> dict:
    """bf16 weight bytes one token has to read, from the shapes."""
    lstm1 = 2 * 4 * H * (E + H)
    lstm2 = 2 * 4 * H * (H + H + DS)
    predict = 2 * V * H
    return {"lstm1_bytes": lstm1, "lstm2_bytes": lstm2,
            "predict_bytes": predict,
            "token_bytes": lstm1 + lstm2 + predict}


def _build(T, N, device, like=None):
    net = Net(text_format.parse(net_text(T, N), caffe_pb.NetParameter),
              caffe_pb.NetState(phase=caffe_pb.Phase.TEST), device=device,
              dtype=torch.bfloat16)
    if like is not None:
        net.share_trained_layers_with(like)
    else:
        g = torch.Generator().manual_seed(1)
        for layer in net.layers:
            for b in layer.blobs:
                w = (torch.rand(b.shape, generator=g) * 2 - 1) * 0.05
                b.data.copy_(w.to(device))
    return net


def _feed(net, T, N, g):
    d = net.device
    cont = torch.ones(T, N)
    cont[0] = 0
    net.blob_by_name("cont_sentence").data = cont.to(d, torch.bfloat16)
    net.blob_by_name("input_sentence").data = torch.randint(
        1, V, (T, N), generator=g).float().to(d)
    net.blob_by_name("image_features").data = \
        (torch.rand(N, DS, generator=g) * 2 - 1).to(d, torch.bfloat16)


def _window(fn, iters: int) -> float:
    """Milliseconds per call over `iters` calls, by device events."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _layer_shares(net, iters=200) -> dict:
    """ms per forward of each layer of the step net, timed one by one."""
    out = {}
    for layer, bot, top in zip(net.layers, net.layer_bottoms,
                               net.layer_tops):
        fn = lambda: layer.forward(bot, top)          # noqa: E731
        _window(fn, 20)
        out[layer.name] = round(_window(fn, iters), 4)
    return out


def bench_n(N, device, window_s, reps) -> dict:
    g = torch.Generator().manual_seed(2)
    unrolled = _build(TOKENS, N, device)
    step = _build(1, N, device, like=unrolled)
    step.set_recurrent_stateful(True)
    _feed(unrolled, TOKENS, N, g)
    _feed(step, 1, N, g)
    step.blob_by_name("cont_sentence").data.fill_(1.0)

    def run_unrolled():
        unrolled.forward(read_loss=False)

    def run_step():
        step.forward(read_loss=False)

    methods = {"unrolled": (run_unrolled, None),
               "gemm": (run_step, "0"), "fused": (run_step, "1")}
    out = {"N": N}
    iters = {}
    for name, (fn, flag) in methods.items():      # warm-up + window sizing
        if flag is not None:
            os.environ["COS_LSTM_STEP"] = flag
        _window(fn, 5)
        per = _window(fn, 20)
        iters[name] = max(20, int(window_s * 1e3 / max(per, 1e-3)))
        if flag is not None:
            out[f"{name}_route"] = step.layer_by_name("lstm2").step_route
    ms = {name: [] for name in methods}
    for _ in range(reps):                         # alternate the methods
        for name, (fn, flag) in methods.items():
            if flag is not None:
                os.environ["COS_LSTM_STEP"] = flag
            ms[name].append(_window(fn, iters[name]))
    for name, v in ms.items():
        out[f"{name}_ms_per_token"] = round(statistics.median(v), 4)
        out[f"{name}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        out[f"{name}_iters"] = iters[name]
    wb = weight_bytes()
    out.update(wb)
    out["fused_end_to_end_bytes_per_s"] = round(
        wb["token_bytes"] / (out["fused_ms_per_token"] * 1e-3))
    out["fused_share_of_hbm_ceiling"] = round(
        out["fused_end_to_end_bytes_per_s"] / HBM_CEILING, 4)
    os.environ["COS_LSTM_STEP"] = "1"
    out["fused_layer_ms"] = _layer_shares(step)
    lstm_ms = out["fused_layer_ms"]["lstm1"] + out["fused_layer_ms"]["lstm2"]
    out["fused_lstm_layers_bytes_per_s"] = round(
        (wb["lstm1_bytes"] + wb["lstm2_bytes"]) / (lstm_ms * 1e-3))
    os.environ["COS_LSTM_STEP"] = "0"
    out["gemm_layer_ms"] = _layer_shares(step)
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--window", type=float, default=0.5,
                    help="seconds of device work per timed window")
    ap.add_argument("--reps", type=int, default=5,
                    help="timed windows per method")
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 4, 16, 64])
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs a GPU: none is present")
    device = torch.device("cuda:0")
    prev = os.environ.get("COS_LSTM_STEP")
    try:
        for n in args.streams:
            res = {"bench": "caption_decode",
                   "device": torch.cuda.get_device_name(0), "dtype": "bf16",
                   "tokens_unrolled": TOKENS}
            res.update(bench_n(n, device, args.window, args.reps))
            print(json.dumps(res), flush=True)
    finally:
        if prev is None:
            os.environ.pop("COS_LSTM_STEP", None)
        else:
            os.environ["COS_LSTM_STEP"] = prev


if __name__ == "__main__":
    main()
