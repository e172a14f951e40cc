"""Pod runner — the container entrypoint for process-backed pods.

When the ProcessKubelet (kubelet/process.py) runs a pod as a real OS process, this
module is the "container image": it receives the injected GROVE_* env contract
(api/common/constants parity), runs grove-initc against the HTTP apiserver when the
pod's clique has startup dependencies, executes the payload on the assigned GPU
(HIP_VISIBLE_DEVICES set by the kubelet), and exits 0 on success — exactly the
lifecycle a real inference container sees under the reference stack.
"""
from __future__ import annotations

import json
import os
import sys
from typing import Optional, Tuple

GEMM_DEFAULT_SHAPE = "512x512x512x1"  # a pod with no shape annotation stays small


def payload_dims(payload: str, shape: Optional[str]) -> Tuple[int, ...]:
    """Dims for run_payload_descriptor from the GROVE_PAYLOAD / GROVE_PAYLOAD_SHAPE
    env contract, through the parser the in-process kubelet uses. An unset shape is
    the runner's own small default for gemm and the kind's default otherwise; an
    unknown kind has no dims and runs nothing."""
    from .gpunode import PAYLOAD_KINDS, parse_payload_shape
    if payload not in PAYLOAD_KINDS:
        return ()
    if not shape:
        shape = GEMM_DEFAULT_SHAPE if payload == "gemm" else ""
    return parse_payload_shape(payload, shape)


def main() -> int:
    pcs = os.environ.get("GROVE_PCS_NAME", "?")
    pclq = os.environ.get("GROVE_PCLQ_NAME", "?")
    idx = os.environ.get("GROVE_PCLQ_POD_INDEX", "?")
    server = os.environ.get("GROVE_API_SERVER")
    podgang = os.environ.get("GROVE_PODGANG_NAME")
    parents = os.environ.get("GROVE_STARTS_AFTER", "")  # "fqn:min,fqn:min"
    namespace = os.environ.get("GROVE_NAMESPACE", "default")

    print(f"podrunner: {pclq}/{idx} of {pcs} starting", flush=True)

    if parents and server and podgang:
        from ..initc import wait_for_parents, parse_podcliques
        specs = parse_podcliques(parents.split(","))
        ok = wait_for_parents(namespace, podgang, specs, server=server,
                              timeout=float(os.environ.get("GROVE_INITC_TIMEOUT",
                                                           "120")),
                              poll=0.1)
        if not ok:
            print("podrunner: initc timed out", file=sys.stderr, flush=True)
            return 1
        print("podrunner: startup dependencies satisfied", flush=True)

    payload = os.environ.get("GROVE_PAYLOAD", "gemm")
    if payload != "none":
        from .gpunode import run_payload_descriptor
        dims = payload_dims(payload, os.environ.get("GROVE_PAYLOAD_SHAPE"))
        # HIP_VISIBLE_DEVICES is set by the kubelet → device 0 is OUR gpu
        metrics = run_payload_descriptor(payload, dims, 0)
        print("podrunner: payload done", json.dumps(metrics), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
