"""Stateful and expose_hidden LSTM semantics on CPU fp32: token-by-token
decode must compute what the unrolled net computes."""

import os

import numpy as np
import pytest
import torch

from caffeonspark_amd.core.blob import Blob
from caffeonspark_amd.core.net import Net
from caffeonspark_amd.proto import caffe_pb, text_format
from test_layers import make_layer, run_grad_check

V, E, H, DS = 11, 8, 8, 8
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "reference",
                       "data", "lrcn_word_to_preds.deploy.prototxt")
FILL = 'weight_filler { type: "uniform" min: -0.4 max: 0.4 }'
# the project's fp32-chain precedent
RTOL, ATOL = 1e-5, 1e-6


def tiny_text(T, N):
    return f'''
name: "tiny"
input: "cont_sentence" input_shape {{ dim: {T} dim: {N} }}
input: "input_sentence" input_shape {{ dim: {T} dim: {N} }}
input: "image_features" input_shape {{ dim: {N} dim: {DS} }}
layer {{ name: "embedding" type: "Embed" bottom: "input_sentence"
  top: "emb" embed_param {{ input_dim: {V} num_output: {E} bias_term: false
    {FILL} }} }}
layer {{ name: "lstm1" type: "LSTM" bottom: "emb" bottom: "cont_sentence"
  top: "lstm1" recurrent_param {{ num_output: {H} {FILL}
    bias_filler {{ type: "uniform" min: -0.2 max: 0.2 }} }} }}
layer {{ name: "lstm2" type: "LSTM" bottom: "lstm1" bottom: "cont_sentence"
  bottom: "image_features" top: "lstm2"
  recurrent_param {{ num_output: {H} {FILL}
    bias_filler {{ type: "uniform" min: -0.2 max: 0.2 }} }} }}
layer {{ name: "predict" type: "InnerProduct" bottom: "lstm2" top: "predict"
  inner_product_param {{ axis: 2 num_output: {V} {FILL} }} }}
layer {{ name: "probs" type: "Softmax" bottom: "predict" top: "probs"
  softmax_param {{ axis: 2 }} }}
'''


def tiny_net(T, N, like=None):
    net = Net(text_format.parse(tiny_text(T, N), caffe_pb.NetParameter),
              caffe_pb.NetState(phase=caffe_pb.Phase.TEST), seed=3)
    if like is not None:
        for a, b in zip(net.layers, like.layers):
            for pa, pb in zip(a.blobs, b.blobs):
                pa.data.copy_(pb.data)
    return net


def feed(net, cont, words, feats):
    net.blob_by_name("cont_sentence").data = cont.clone()
    net.blob_by_name("input_sentence").data = words.clone()
    net.blob_by_name("image_features").data = feats.clone()
    net.forward()
    return net.blob_by_name("probs").data.clone()


@pytest.fixture(scope="module")
def unrolled():
    """One T=5, N=3 forward: cont[0] = 0 and stream 1 restarts at t = 3."""
    g = torch.Generator().manual_seed(11)
    T, N = 5, 3
    cont = torch.ones(T, N)
    cont[0] = 0
    cont[3, 1] = 0
    words = torch.randint(0, V, (T, N), generator=g).float()
    feats = torch.randn(N, DS, generator=g)
    net = tiny_net(T, N)
    return dict(net=net, cont=cont, words=words, feats=feats,
                probs=feed(net, cont, words, feats))


def test_step_equals_unroll(unrolled):
    u = unrolled
    step = tiny_net(1, 3, like=u["net"])
    step.set_recurrent_stateful(True)
    for t in range(5):
        p = feed(step, u["cont"][t:t + 1], u["words"][t:t + 1], u["feats"])
        assert p.shape == (1, 3, V)
        torch.testing.assert_close(p[0], u["probs"][t], rtol=RTOL, atol=ATOL,
                                   msg=lambda m, t=t: f"step {t}: {m}")


def test_default_is_not_stateful(unrolled):
    u = unrolled
    net = tiny_net(1, 3, like=u["net"])
    assert not any(l.stateful for l in net._recurrent_layers())
    cont = torch.ones(1, 3)
    a = feed(net, cont, u["words"][1:2], u["feats"])
    b = feed(net, cont, u["words"][1:2], u["feats"])
    assert torch.equal(a, b)
    # and it is the zero-start answer
    z = tiny_net(1, 3, like=u["net"])
    assert torch.equal(a, feed(z, torch.zeros(1, 3), u["words"][1:2],
                               u["feats"]))


# ------------------------------------------------------------ expose_hidden

def exposed_layer(static, stateful=False):
    layer = make_layer(f'''
        name: "l" type: "LSTM" bottom: "x" bottom: "cont"
        {'bottom: "xs"' if static else ''} bottom: "h0" bottom: "c0"
        top: "h" top: "hT" top: "cT"
        recurrent_param {{ num_output: {H} expose_hidden: true {FILL}
          bias_filler {{ type: "uniform" min: -0.2 max: 0.2 }} }}''')
    layer.stateful = stateful
    return layer


def blobs_of(*tensors):
    out = []
    for t in tensors:
        b = Blob(t.shape)
        b.data = t.clone()
        out.append(b)
    return out


def exposed_inputs(T, N, D, static, seed=5):
    g = torch.Generator().manual_seed(seed)
    cont = torch.ones(T, N)
    cont[0, 0] = 0
    if T > 3:
        cont[3, 1] = 0
    ins = [torch.randn(T, N, D, generator=g), cont]
    if static:
        ins.append(torch.randn(N, DS, generator=g))
    ins += [torch.randn(1, N, H, generator=g) * 0.5,
            torch.randn(1, N, H, generator=g) * 0.5]
    return ins


@pytest.mark.parametrize("static", [False, True])
def test_expose_hidden_shapes_and_bottom_order(static):
    T, N, D = 4, 3, 6
    layer = exposed_layer(static)
    bottom = blobs_of(*exposed_inputs(T, N, D, static))
    top = [Blob([0]) for _ in range(3)]
    layer.setup(bottom, top)
    assert layer.static == static
    assert len(layer.blobs) == (4 if static else 3)
    if static:
        assert layer.blobs[3].shape == [4 * H, DS]
    layer.forward(bottom, top)
    assert top[0].shape == [T, N, H]
    assert top[1].shape == [1, N, H] and top[2].shape == [1, N, H]
    assert top[2].data.dtype == torch.float32
    assert torch.equal(top[1].data[0], top[0].data[-1])
    # h_0 / c_0 are the LAST two bottoms: zeroing them changes the output
    ref = top[0].data.clone()
    bottom[-2].data = torch.zeros(1, N, H)
    bottom[-1].data = torch.zeros(1, N, H)
    layer.forward(bottom, top)
    assert not torch.equal(top[0].data, ref)


def test_expose_hidden_wrong_counts():
    layer = make_layer(f'''
        name: "l" type: "LSTM" bottom: "x" bottom: "cont" bottom: "h0"
        top: "h" top: "hT" top: "cT"
        recurrent_param {{ num_output: {H} expose_hidden: true }}''')
    with pytest.raises(ValueError):
        layer.setup(blobs_of(torch.zeros(2, 1, 4), torch.zeros(2, 1),
                             torch.zeros(1, 1, H)),
                    [Blob([0]) for _ in range(3)])


def test_expose_hidden_chain_equals_whole():
    """T=2 then T=3 chained through h_T/c_T equals one T=5 forward."""
    T, N, D = 5, 3, 6
    ins = exposed_inputs(T, N, D, True)
    x, cont, xs, h0, c0 = ins
    layer = exposed_layer(True)
    bottom = blobs_of(*ins)
    top = [Blob([0]) for _ in range(3)]
    layer.setup(bottom, top)
    layer.forward(bottom, top)
    whole = [t.data.clone() for t in top]
    b1 = blobs_of(x[:2], cont[:2], xs, h0, c0)
    layer.forward(b1, top)
    first = top[0].data.clone()
    b2 = blobs_of(x[2:], cont[2:], xs, top[1].data, top[2].data)
    layer.forward(b2, top)
    got = torch.cat([first, top[0].data], dim=0)
    torch.testing.assert_close(got, whole[0], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(top[1].data, whole[1], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(top[2].data, whole[2], rtol=RTOL, atol=ATOL)


def test_exposed_stepping_bit_equals_carried():
    T, N, D = 5, 3, 6
    x, cont, xs, _, _ = exposed_inputs(T, N, D, True)
    exp = exposed_layer(True)
    car = make_layer(f'''
        name: "l" type: "LSTM" bottom: "x" bottom: "cont" bottom: "xs"
        top: "h" recurrent_param {{ num_output: {H} }}''')
    h = torch.zeros(1, N, H)
    c = torch.zeros(1, N, H)
    etop = [Blob([0]) for _ in range(3)]
    ctop = [Blob([0])]
    exp.setup(blobs_of(x[:1], cont[:1], xs, h, c), etop)
    car.setup(blobs_of(x[:1], cont[:1], xs), ctop)
    car.stateful = True
    for pe, pc in zip(exp.blobs, car.blobs):
        pc.data.copy_(pe.data)
    for t in range(T):
        exp.forward(blobs_of(x[t:t + 1], cont[t:t + 1], xs, h, c), etop)
        car.forward(blobs_of(x[t:t + 1], cont[t:t + 1], xs), ctop)
        assert torch.equal(etop[0].data, ctop[0].data), f"step {t}"
        h, c = etop[1].data, etop[2].data
    assert torch.equal(car._state[0], h[0]) and torch.equal(car._state[1],
                                                            c[0])


class _AllTops:
    """Presents an expose_hidden layer's three tops as one [T+2, N, H] top,
    so the project's grad-check helper (which seeds the first top only)
    drives non-zero h_T and c_T diffs as well."""

    def __init__(self, layer):
        self.layer = layer
        self.param = caffe_pb.LayerParameter(top=["all"])
        self.tops = [Blob([0]) for _ in range(3)]

    @property
    def blobs(self):
        return self.layer.blobs

    def setup(self, bottom, top):
        self.layer.setup(bottom, self.tops)

    def forward(self, bottom, top):
        self.layer.forward(bottom, self.tops)
        top[0].data = torch.cat([t.data for t in self.tops], dim=0)

    def backward(self, top, propagate_down, bottom):
        T = self.tops[0].data.shape[0]
        d = top[0].diff
        self.tops[0].diff = d[:T]
        self.tops[1].diff = d[T:T + 1]
        self.tops[2].diff = d[T + 1:]
        self.layer.backward(self.tops, propagate_down, bottom)


@pytest.mark.parametrize("static", [False, True])
def test_expose_hidden_gradients(static):
    T, N, D = 4, 3, 6
    ins = exposed_inputs(T, N, D, static)
    grad = [True, False] + ([True] if static else []) + [True, True]
    run_grad_check(_AllTops(exposed_layer(static)), ins, grad_bottoms=grad)


# --------------------------------------------------------------- lifecycle

def test_state_resets_when_n_changes_and_on_request(unrolled):
    u = unrolled
    net = tiny_net(1, 3, like=u["net"])
    net.set_recurrent_stateful(True)
    ones = torch.ones(1, 3)
    w = u["words"][1:2]
    fresh = feed(net, ones, w, u["feats"])       # zero state, cont = 1
    carried = feed(net, ones, w, u["feats"])
    assert not torch.equal(fresh, carried)
    net.reset_recurrent_state()
    assert torch.equal(feed(net, ones, w, u["feats"]), fresh)
    # N 3 -> 2 -> 3: each change starts from zeros again
    two = feed(net, ones[:, :2], w[:, :2], u["feats"][:2])
    torch.testing.assert_close(two, fresh[:, :2], rtol=RTOL, atol=ATOL)
    assert torch.equal(feed(net, ones, w, u["feats"]), fresh)
    lstm = net.layer_by_name("lstm1")
    assert lstm._state[0].dtype == torch.float32      # compute dtype
    assert lstm._state[1].dtype == torch.float32
    lstm.reset_state()
    assert lstm._state is None


def test_stateful_backward_raises(unrolled):
    layer = make_layer(f'''
        name: "l" type: "LSTM" bottom: "x" bottom: "cont" top: "h"
        recurrent_param {{ num_output: {H} }}''')
    bottom = blobs_of(torch.randn(2, 3, 6), torch.ones(2, 3))
    top = [Blob([0])]
    layer.setup(bottom, top)
    layer.stateful = True
    layer.forward(bottom, top)
    top[0].diff = torch.ones_like(top[0].data)
    with pytest.raises(RuntimeError, match="stateful"):
        layer.backward(top, [True, False], bottom)


def test_expose_hidden_with_stateful_raises():
    layer = exposed_layer(False, stateful=True)
    bottom = blobs_of(*exposed_inputs(2, 3, 6, False))
    top = [Blob([0]) for _ in range(3)]
    layer.setup(bottom, top)
    layer.stateful = True
    with pytest.raises(RuntimeError, match="expose_hidden"):
        layer.forward(bottom, top)


# ------------------------------------------------------------------ pycaffe

def test_pycaffe_steps_the_deploy_fixture(tmp_path):
    """The reference's word_to_preds deploy net, stepped through the pycaffe
    surface at 2 streams, against a T=3 build of the same text."""
    import caffeonspark_amd.pycaffe as caffe
    T, N = 3, 2
    with open(FIXTURE) as fh:
        text = fh.read()
    assert text.count("dim: 1 dim: 1000") == 2
    unrolled_text = text.replace("dim: 1 dim: 1000", f"dim: {T} dim: {N}") \
        .replace("dim: 1000 dim: 1000", f"dim: {N} dim: 1000")
    path = tmp_path / "unrolled.prototxt"
    path.write_text(unrolled_text)
    step = caffe.Net(FIXTURE, None, caffe.TEST)
    whole = caffe.Net(str(path), None, caffe.TEST, stateful_recurrent=False)
    step.blobs["cont_sentence"].reshape(1, N)
    step.blobs["input_sentence"].reshape(1, N)
    step.blobs["image_features"].reshape(N, 1000)
    assert step.reshape() is None
    assert step.blobs["image_features"].shape == (N, 1000)
    rng = np.random.RandomState(7)
    for name, views in step.params.items():
        for i, v in enumerate(views):
            w = rng.uniform(-0.05, 0.05, size=v.shape).astype(np.float32)
            v.data = w
            whole.params[name][i].data = w
    cont = np.ones((T, N), np.float32)
    cont[0] = 0
    words = rng.randint(0, 8801, size=(T, N)).astype(np.float32)
    feats = rng.uniform(-1, 1, size=(N, 1000)).astype(np.float32)
    want = whole.forward(cont_sentence=cont, input_sentence=words,
                         image_features=feats)["probs"]
    for t in range(T):
        got = step.forward(cont_sentence=cont[t:t + 1],
                           input_sentence=words[t:t + 1],
                           image_features=feats)["probs"]
        assert got.shape == (1, N, 8801)
        np.testing.assert_allclose(got[0], want[t], rtol=RTOL, atol=ATOL,
                                   err_msg=f"step {t}")
    # the carried state is what made steps 1 and 2 right
    step.reset_recurrent_state()
    again = step.forward(cont_sentence=cont[2:3], input_sentence=words[2:3],
                         image_features=feats)["probs"]
    assert not np.allclose(again[0], want[2], rtol=1e-3, atol=0)


# ---------------------------------------------------------------- captioner

def _tiny_captioner(tmp_path, n):
    from caffeonspark_amd.tools.captioner import Captioner
    from caffeonspark_amd.proto import write_binary_proto
    proto = tmp_path / "step.prototxt"
    proto.write_text(tiny_text(1, n))
    src = tiny_net(1, n)
    weights = tmp_path / "tiny.caffemodel"
    write_binary_proto(str(weights), src.to_proto())
    vocab = ["<eos>"] + [f"w{i}" for i in range(1, V)]
    cap = Captioner(str(weights), None, str(proto), vocab, seed=4)
    return cap, src


def test_captioner_greedy_equals_unrolled_decode(tmp_path):
    n, max_len = 3, 7
    cap, src = _tiny_captioner(tmp_path, n)
    assert cap.caption_batch_size == n
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(n, DS, generator=g)
    tokens, probs = cap.sample_captions(feats.numpy(), max_length=max_len)
    # the parent-commit method: re-run the whole unrolled net per token
    net = tiny_net(max_len, n, like=src)
    cont = torch.ones(max_len, n)
    cont[0] = 0
    words = torch.zeros(max_len, n)
    want = [[] for _ in range(n)]
    done = [False] * n
    for t in range(max_len):
        p = feed(net, cont, words, feats)
        nxt = p[t].argmax(dim=1)
        for i in range(n):
            if not done[i]:
                want[i].append(int(nxt[i]))
                done[i] = int(nxt[i]) == 0
        if t + 1 < max_len:
            words[t + 1] = nxt.float()
        if all(done):
            break
    assert tokens == want
    assert all(len(t) == len(p) for t, p in zip(tokens, probs))
    assert all(0.0 < q <= 1.0 for p in probs for q in p)
    s = cap.sentence(tokens[0])
    assert s == " ".join(f"w{i}" for i in tokens[0] if i != 0)
    # a stream's list ends at its first EOS
    for t in tokens:
        assert 0 not in t[:-1]


def test_captioner_sampling_is_seeded(tmp_path):
    cap_a, _ = _tiny_captioner(tmp_path, 2)
    cap_b, _ = _tiny_captioner(tmp_path, 2)
    feats = np.linspace(-1, 1, DS, dtype=np.float32)    # one descriptor
    a = [cap_a.sample_captions(feats, temp=1.5, max_length=6)[0]
         for _ in range(2)]
    b = [cap_b.sample_captions(feats, temp=1.5, max_length=6)[0]
         for _ in range(2)]
    assert a == b
    cap_a.set_caption_batch_size(4)
    assert cap_a.caption_batch_size == 4
    assert len(cap_a.sample_captions(feats, max_length=3)[0]) == 4


# ------------------------------------------------------------------ example

IMAGE_NET = f'''
name: "tiny_image"
input: "data" input_shape {{ dim: 1 dim: 3 dim: 227 dim: 227 }}
layer {{ name: "gap" type: "Pooling" bottom: "data" top: "gap"
  pooling_param {{ pool: AVE global_pooling: true }} }}
layer {{ name: "fc8" type: "InnerProduct" bottom: "gap" top: "fc8"
  inner_product_param {{ num_output: {DS} {FILL} }} }}
'''


def test_example_step_decoding_flags(tmp_path):
    """examples/image_caption.py with -lstmNet / -imageNet decodes through
    the Captioner; one of the two flags alone is an error."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples"))
    import image_caption
    from caffeonspark_amd.api import Config
    from caffeonspark_amd.proto import write_binary_proto
    from caffeonspark_amd.tools.vocab import Vocab
    Image = pytest.importorskip("PIL.Image")
    img = (np.random.RandomState(0).rand(64, 64, 3) * 255).astype("uint8")
    p = str(tmp_path / "cat.jpg")
    Image.fromarray(img).save(p)
    lstm = tmp_path / "lstm.prototxt"
    lstm.write_text(tiny_text(1, 1))
    inet = tmp_path / "image.prototxt"
    inet.write_text(IMAGE_NET)
    both = tiny_net(1, 1).to_proto()
    image_net = Net(text_format.parse(IMAGE_NET, caffe_pb.NetParameter),
                    caffe_pb.NetState(phase=caffe_pb.Phase.TEST), seed=5)
    both.layer = list(both.layer) + list(image_net.to_proto().layer)
    weights = tmp_path / "both.caffemodel"
    write_binary_proto(str(weights), both)
    vocab = tmp_path / "vocab.json"
    Vocab(["<eos>"] + [f"w{i}" for i in range(1, V)]).save(str(vocab))
    conf = Config(["-weights", str(weights), "-vocabDir", str(vocab)])
    conf.device = torch.device("cpu")
    res = image_caption.caption_images_step(conf, [p], str(lstm), str(inet),
                                            max_len=4)
    assert len(res) == 1 and res[0][0] == p
    words = res[0][1].split()
    assert len(words) <= 4 and all(w.startswith("w") for w in words)
    with pytest.raises(SystemExit, match="go together"):
        image_caption.main(["-lstmNet", str(lstm), "-imageRoot",
                            str(tmp_path)])
