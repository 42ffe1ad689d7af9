"""HDF5 snapshot format, vocab/coco tools, mini-cluster CLI pieces."""

import json
import os

import numpy as np
import torch

from caffeonspark_amd.proto import caffe_pb, text_format
from caffeonspark_amd.utils import hdf5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hdf5_roundtrip_nested(tmp_path):
    root = hdf5.H5Group()
    root.attrs["iter"] = 7
    root.attrs["learned_net"] = "abc.h5"
    g = hdf5.H5Group()
    root["data"] = g
    g["layer.with.dots"] = hdf5.H5Group()
    g["layer.with.dots"]["0"] = np.random.randn(3, 4, 5).astype(np.float32)
    f = str(tmp_path / "t.h5")
    hdf5.save(f, root)
    r = hdf5.load(f)
    assert r.attrs["iter"] == 7
    np.testing.assert_allclose(r["data"]["layer.with.dots"]["0"],
                               g["layer.with.dots"]["0"])


def test_hdf5_string_attr_keeps_trailing_nul(tmp_path):
    """A string attribute is stored with exactly one terminator, so values
    that are empty or end in NUL themselves read back unchanged (the case
    the hdf5 fuzz test only hits on some draws)."""
    for i, val in enumerate(["", "\x00", "a\x00\x00", "abc.h5"]):
        root = hdf5.H5Group()
        root.attrs["note"] = val
        f = str(tmp_path / f"s{i}.h5")
        hdf5.save(f, root)
        assert hdf5.load(f).attrs["note"] == val


def test_hdf5_solver_snapshot_restore(tmp_path):
    """cifar10_quick-style HDF5 snapshot (snapshot_format: HDF5) round-trip
    through the Solver."""
    from caffeonspark_amd.core.solver import Solver

    sp = text_format.parse_file(
        os.path.join(ROOT, "caffeonspark_amd", "models",
                     "lenet_memory_solver.prototxt"),
        caffe_pb.SolverParameter)
    sp.snapshot_format = caffe_pb.SnapshotFormat.HDF5
    sp.snapshot_prefix = str(tmp_path / "lenet")
    sp.random_seed = 4
    sp.display = 0
    s = Solver(sp, proto_dir=os.path.join(ROOT, "caffeonspark_amd",
                                          "models"))
    x = torch.randn(64, 1, 28, 28)
    y = torch.randint(0, 10, (64,)).float()
    s.net.data_layers()[0].reset(x, y)
    s.step(3)
    model = s.snapshot()
    assert model.endswith(".caffemodel.h5")
    state = s.snapshot_filename("state")
    assert os.path.exists(state)

    s2 = Solver(sp, proto_dir=os.path.join(ROOT, "caffeonspark_amd",
                                           "models"))
    s2.restore(state)
    assert s2.iter == 3
    torch.testing.assert_close(s2.flat_w, s.flat_w)
    torch.testing.assert_close(s2.flat_m, s.flat_m)


def test_vocab_embed():
    from caffeonspark_amd.tools.vocab import Vocab

    v = Vocab.build(["a cat sat", "a dog sat", "a cat ran"], size=10)
    assert len(v) <= 10
    ids = v.embed("a cat flew", 6)
    assert len(ids) == 6
    assert ids[-3] == 0 or 0 in ids      # EOS present
    assert ids[-1] == -1                 # padded with ignore label
    # unk maps to the unk id
    assert ids[2] == v.index["<unk>"]


def test_coco_pipeline(tmp_path):
    from caffeonspark_amd.tools.coco import coco_to_dataframe, embed_captions

    # synthesize a tiny COCO-style dataset
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    from PIL import Image
    for i in range(3):
        Image.new("RGB", (32, 32), (i * 40, 100, 50)).save(
            str(img_dir / f"im{i}.jpg"))
    doc = {
        "images": [{"id": i, "file_name": f"im{i}.jpg"} for i in range(3)],
        "annotations": [
            {"id": 10 + i, "image_id": i, "caption": f"a photo number {i}"}
            for i in range(3)],
    }
    cj = tmp_path / "captions.json"
    cj.write_text(json.dumps(doc))
    df1 = str(tmp_path / "capdf.parquet")
    n = coco_to_dataframe(str(cj), str(img_dir), df1)
    assert n == 3
    df2 = str(tmp_path / "embedded.parquet")
    n2 = embed_captions(df1, str(tmp_path / "vocab.json"), df2,
                        caption_length=8, vocab_size=50)
    assert n2 == 3
    import pyarrow.parquet as pq
    t = pq.read_table(df2)
    assert set(t.schema.names) >= {"data", "label", "input_sentence",
                                   "target_sentence", "cont_sentence"}
    row_inp = t.column("input_sentence")[0].as_py()
    assert len(row_inp) == 9 and row_inp[0] == 0


def test_mini_cluster_single(tmp_path):
    """mini_cluster with -cluster 1 runs the train CLI end to end."""
    from tests.test_e2e_pipeline import LENET_NET, SOLVER, \
        make_synthetic_lmdb

    make_synthetic_lmdb(str(tmp_path / "train_lmdb"), 400, 3)
    make_synthetic_lmdb(str(tmp_path / "test_lmdb"), 100, 4)
    (tmp_path / "net.prototxt").write_text(
        LENET_NET.format(train=str(tmp_path / "train_lmdb"),
                         test=str(tmp_path / "test_lmdb")))
    (tmp_path / "solver.prototxt").write_text(
        SOLVER.format(net=str(tmp_path / "net.prototxt"), test_interval=0,
                      max_iter=10, prefix=str(tmp_path / "mc")))
    from caffeonspark_amd.data.processor import CaffeProcessor
    from caffeonspark_amd.tools import mini_cluster

    CaffeProcessor.reset_instance()
    mini_cluster.main(["-cluster", "1", "-conf",
                       str(tmp_path / "solver.prototxt"), "-train"])
    snaps = [f for f in os.listdir(tmp_path) if f.endswith(".caffemodel")]
    assert snaps
    CaffeProcessor.reset_instance()


def test_pycaffe_shim(tmp_path):
    """pycaffe-style inference API over our Net."""
    import caffeonspark_amd.pycaffe as caffe

    proto = tmp_path / "deploy.prototxt"
    proto.write_text("""
    layer { name: "data" type: "Input" top: "data"
            input_param { shape { dim: 2 dim: 4 } } }
    layer { name: "ip" type: "InnerProduct" bottom: "data" top: "ip"
            inner_product_param { num_output: 3
              weight_filler { type: "xavier" } } }
    layer { name: "prob" type: "Softmax" bottom: "ip" top: "prob" }
    """)
    net = caffe.Net(str(proto), None, caffe.TEST)
    x = np.random.randn(2, 4).astype(np.float32)
    out = net.forward(data=x)
    assert "prob" in out
    np.testing.assert_allclose(out["prob"].sum(axis=1), [1.0, 1.0],
                               rtol=1e-4)
    assert net.params["ip"][0].shape == (3, 4)


def test_simulator_runs(capsys):
    """Simulator (reference Simulator.java analog): decode/transform
    throughput driver completes and reports a rate."""
    from caffeonspark_amd.tools import simulator
    simulator.main(["-iters", "8", "-batch", "4", "-size", "32"])
    out = capsys.readouterr().out
    assert "images/sec" in out or "img/s" in out or out.strip()


def test_all_modules_import():
    """Every package module imports cleanly (catches stale references
    after refactors)."""
    import importlib
    import pkgutil

    import caffeonspark_amd
    skipped = []
    for m in pkgutil.walk_packages(caffeonspark_amd.__path__,
                                   prefix="caffeonspark_amd."):
        try:
            importlib.import_module(m.name)
        except ImportError as e:   # optional deps only
            skipped.append((m.name, str(e)))
    assert not skipped, f"import failures: {skipped}"


def test_display_utils():
    """DisplayUtils analog renders an image/label table."""
    import pandas as pd

    from caffeonspark_amd.api.display import df_to_html
    df = pd.DataFrame([{"data": b"xx", "label": 3},
                       {"data": None, "label": 1}])
    html = df_to_html(df, text_col="label")
    assert "<table>" in html and "<img" in html and ">3<" in html


def test_pycaffe_backward_and_save(tmp_path):
    """pycaffe shim: backward returns input gradients; save writes a
    loadable .caffemodel."""
    import numpy as np

    import caffeonspark_amd.pycaffe as caffe
    from caffeonspark_amd.proto import caffe_pb

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proto = os.path.join(root, "caffeonspark_amd", "models",
                         "lenet_memory_train_test.prototxt")
    net = caffe.Net(proto, phase=caffe_pb.Phase.TRAIN)
    dl = net._net.data_layers()[0]
    import torch
    dl.reset(torch.randn(4, 1, 28, 28), torch.randint(0, 10, (4,)).float())
    net._net.forward()
    grads = net.backward()
    assert any(np.abs(g).sum() > 0 for g in grads.values())
    out = str(tmp_path / "m.caffemodel")
    net.save(out)
    net2 = caffe.Net(proto, weights=out, phase=caffe_pb.Phase.TRAIN)
    np.testing.assert_allclose(net.params["ip2"][0].data,
                               net2.params["ip2"][0].data)
    assert "loss" in net.outputs or net.outputs


def test_time_net_per_layer(capsys):
    """caffe-time analog: per-layer fwd/bwd timing table."""
    import os

    from caffeonspark_amd.tools import time_net
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    time_net.main(["-conf",
                   os.path.join(root, "caffeonspark_amd", "models",
                                "lenet_memory_solver.prototxt"),
                   "-iters", "2", "-batch", "8"])
    out = capsys.readouterr().out
    assert "TOTAL" in out
    assert "conv1" in out and "ip2" in out
