"""decode_batch payload plumbing (CPU): shape grammar, the shared shape parser, the
CPU fallback, the pod runner's dims and the disaggregated-batched sample."""
import os

import pytest

from grove_amd.api import constants as c
from grove_amd.kubelet import gpunode, podrunner

SAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "samples")


def _pod(kind=None, shape=None):
    ann = {}
    if kind is not None:
        ann[gpunode.PAYLOAD_ANNOTATION] = kind
    if shape is not None:
        ann[gpunode.PAYLOAD_SHAPE_ANNOTATION] = shape
    return {"metadata": {"name": "p", "annotations": ann}}


def test_parse_payload_decode_batch():
    assert gpunode.parse_payload(_pod("decode_batch", "256x512x3")) == (
        "decode_batch", (256, 512, 3, 1))
    assert gpunode.parse_payload(_pod("decode_batch", "256x512x3x5")) == (
        "decode_batch", (256, 512, 3, 5))
    assert gpunode.parse_payload(_pod("decode_batch")) == (
        "decode_batch", (16384, 8192, 16, 4))


@pytest.mark.parametrize("shape", ["256x512", "256x512x3x5x7"])
def test_parse_payload_decode_batch_rejects_wrong_field_count(shape):
    with pytest.raises(ValueError):
        gpunode.parse_payload(_pod("decode_batch", shape))


# what parse_payload returned for the existing kinds before the shape parser was
# factored out, written out as literals so the refactor cannot drift
EXISTING = [
    (None, None, ("gemm", (1024, 1024, 1024, 1))),
    ("gemm", None, ("gemm", (1024, 1024, 1024, 1))),
    ("gemm", "512x512x512", ("gemm", (512, 512, 512, 1))),
    ("gemm", "4096x4096x4096x1", ("gemm", (4096, 4096, 4096, 1))),
    ("gemm", "256x384x512x7", ("gemm", (256, 384, 512, 7))),
    (None, "128x256x64x3", ("gemm", (128, 256, 64, 3))),
    ("stream", None, ("stream", (1 << 24, 2))),
    ("stream", "4096", ("stream", (4096, 2))),
    ("stream", "67108864", ("stream", (67108864, 2))),
    ("decode", None, ("decode", (8192, 8192, 4))),
    ("decode", "2048x8192", ("decode", (2048, 8192, 1))),
    ("decode", "16384x8192x4", ("decode", (16384, 8192, 4))),
    ("none", None, ("none", ())),
    ("none", "1x2x3", ("none", ())),
    ("sleep", "12", ("none", ())),
]


@pytest.mark.parametrize("kind,shape,expected", EXISTING)
def test_parse_payload_existing_kinds_unchanged(kind, shape, expected):
    assert gpunode.parse_payload(_pod(kind, shape)) == expected


@pytest.mark.parametrize("kind,shape,expected", [e for e in EXISTING
                                                 if e[0] in gpunode.PAYLOAD_KINDS])
def test_parse_payload_shape_is_what_parse_payload_uses(kind, shape, expected):
    assert gpunode.parse_payload_shape(kind, shape or "") == expected[1]


def test_parse_payload_shape_unknown_kind():
    with pytest.raises(ValueError):
        gpunode.parse_payload_shape("sleep", "")


def test_run_payload_descriptor_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert gpunode.run_payload_descriptor("decode_batch", (256, 512, 3, 1), 0) == {
        "device": "cpu", "kind": "decode_batch"}


def test_podrunner_dims_come_from_shared_parser(monkeypatch):
    assert podrunner.payload_dims("decode_batch", "256x512x3") == (256, 512, 3, 1)
    assert podrunner.payload_dims("decode_batch", "256x512x3x5") == (256, 512, 3, 5)
    assert podrunner.payload_dims("decode_batch", None) == (16384, 8192, 16, 4)
    seen = []
    real = gpunode.parse_payload_shape

    def spy(kind, shape):
        seen.append((kind, shape))
        return real(kind, shape)
    monkeypatch.setattr(gpunode, "parse_payload_shape", spy)
    assert podrunner.payload_dims("decode_batch", "64x512x2") == (64, 512, 2, 1)
    assert seen == [("decode_batch", "64x512x2")]


@pytest.mark.parametrize("payload,shape,expected", [
    # dims the runner's own split("x") produced for these shapes
    ("gemm", None, (512, 512, 512, 1)),
    ("gemm", "512x512x512", (512, 512, 512, 1)),
    ("gemm", "1024x1024x1024x2", (1024, 1024, 1024, 2)),
    ("stream", "4096x3", (4096, 3)),
    # decode could not run through the runner before (its dims never unpacked)
    ("decode", "2048x8192", (2048, 8192, 1)),
    ("decode", "16384x8192x4", (16384, 8192, 4)),
])
def test_podrunner_dims_existing_shapes(payload, shape, expected):
    assert podrunner.payload_dims(payload, shape) == expected


def test_podrunner_stream_single_field_runs_the_same():
    """'N' used to reach run_payload_descriptor as (N,), which then took iters = 2;
    the shared parser spells that default out."""
    assert podrunner.payload_dims("stream", "4096") == (4096, 2)


def test_sample_disaggregated_batched(cluster):
    cluster.store.create({"apiVersion": c.API_VERSION, "kind": c.KIND_CTB,
                          "metadata": {"name": "t"},
                          "spec": {"levels": [
                              {"domain": "host", "key": "kubernetes.io/hostname"}]}})
    cluster.add_virtual_nodes(1, gpus=8, prefix="mi355x")
    with open(os.path.join(SAMPLES, "disaggregated-batched.yaml")) as f:
        cluster.apply(f.read())
    pcs = cluster.wait_pcs_available("disagg-batched", timeout=30)
    assert pcs["status"]["availableReplicas"] == 1
    pods = cluster.store.list("Pod", "default", {c.LABEL_PART_OF: "disagg-batched"})
    assert len(pods) == 8 and {p["spec"]["nodeName"] for p in pods} == {"mi355x-0"}
    decode = [p for p in pods
              if gpunode.parse_payload(p) == ("decode_batch", (16384, 8192, 32, 4))]
    assert len(decode) == 4
