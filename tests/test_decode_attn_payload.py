"""decode_attn payload plumbing (CPU): shape grammar, the existing kinds' grammar
unchanged, the CPU fallback, the pod runner's dims and the disaggregated-longctx
sample."""
import os

import pytest

from grove_amd.api import constants as c
from grove_amd.kubelet import gpunode, podrunner

SAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "samples")
DEFAULT = (64, 8, 8192, 32, 4)


def _pod(kind=None, shape=None):
    ann = {}
    if kind is not None:
        ann[gpunode.PAYLOAD_ANNOTATION] = kind
    if shape is not None:
        ann[gpunode.PAYLOAD_SHAPE_ANNOTATION] = shape
    return {"metadata": {"name": "p", "annotations": ann}}


def test_decode_attn_is_a_payload_kind():
    assert "decode_attn" in gpunode.PAYLOAD_KINDS
    assert gpunode.PAYLOAD_KINDS[:4] == ("gemm", "stream", "decode", "decode_batch")


def test_parse_payload_decode_attn():
    assert gpunode.parse_payload(_pod("decode_attn", "8x1x256x2")) == (
        "decode_attn", (8, 1, 256, 2, 1))
    assert gpunode.parse_payload(_pod("decode_attn", "8x1x256x2x5")) == (
        "decode_attn", (8, 1, 256, 2, 5))
    assert gpunode.parse_payload(_pod("decode_attn")) == ("decode_attn", DEFAULT)
    assert gpunode.parse_payload_shape("decode_attn", "") == DEFAULT


@pytest.mark.parametrize("shape", ["8x1x256", "8x1x256x2x5x7", "8x1x256x2x5x7x9"])
def test_parse_payload_decode_attn_rejects_wrong_field_count(shape):
    with pytest.raises(ValueError):
        gpunode.parse_payload(_pod("decode_attn", shape))


# what parse_payload returns for the kinds that were there before decode_attn,
# written out as literals
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


def test_parse_payload_decode_batch_unchanged():
    assert gpunode.parse_payload(_pod("decode_batch")) == (
        "decode_batch", (16384, 8192, 16, 4))
    assert gpunode.parse_payload(_pod("decode_batch", "256x512x3")) == (
        "decode_batch", (256, 512, 3, 1))
    with pytest.raises(ValueError):
        gpunode.parse_payload(_pod("decode_batch", "256x512x3x5x7"))


def test_run_payload_descriptor_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert gpunode.run_payload_descriptor("decode_attn", (8, 1, 256, 2, 1), 0) == {
        "device": "cpu", "kind": "decode_attn"}


def test_podrunner_dims_come_from_shared_parser(monkeypatch):
    assert podrunner.payload_dims("decode_attn", "8x1x256x2") == (8, 1, 256, 2, 1)
    assert podrunner.payload_dims("decode_attn", "8x1x256x2x5") == (8, 1, 256, 2, 5)
    assert podrunner.payload_dims("decode_attn", None) == DEFAULT
    seen = []
    real = gpunode.parse_payload_shape

    def spy(kind, shape):
        seen.append((kind, shape))
        return real(kind, shape)
    monkeypatch.setattr(gpunode, "parse_payload_shape", spy)
    assert podrunner.payload_dims("decode_attn", "16x2x64x3") == (16, 2, 64, 3, 1)
    assert seen == [("decode_attn", "16x2x64x3")]


def test_sample_disaggregated_longctx(cluster):
    cluster.store.create({"apiVersion": c.API_VERSION, "kind": c.KIND_CTB,
                          "metadata": {"name": "t"},
                          "spec": {"levels": [
                              {"domain": "host", "key": "kubernetes.io/hostname"}]}})
    cluster.add_virtual_nodes(1, gpus=8, prefix="mi355x")
    with open(os.path.join(SAMPLES, "disaggregated-longctx.yaml")) as f:
        cluster.apply(f.read())
    pcs = cluster.wait_pcs_available("disagg-longctx", timeout=30)
    assert pcs["status"]["availableReplicas"] == 1
    pods = cluster.store.list("Pod", "default", {c.LABEL_PART_OF: "disagg-longctx"})
    assert len(pods) == 8 and {p["spec"]["nodeName"] for p in pods} == {"mi355x-0"}
    decode = [p for p in pods if gpunode.parse_payload(p) == ("decode_attn", DEFAULT)]
    assert len(decode) == 4
