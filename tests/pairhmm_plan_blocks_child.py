"""Child process of tests/test_pairhmm_planned_pass.py: the named batches of tests/planned_shapes.py on a plain fp32
context under whatever GKLHIP_PLAN_BLOCKS the parent put into the environment (read once per process), as a host call
and as a device-resident call.  Prints one JSON line: per batch the SHA-256 digests of `out`, the raw fp32 sums, the raw
fp64 sums of the flagged pairs and the flags.

usage: python -m tests.pairhmm_plan_blocks_child --names B:1025,D [--fma 1]"""
import argparse
import json
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", required=True)
    ap.add_argument("--fma", type=int, default=1)
    a = ap.parse_args()
    import torch
    from gkl_amd import native
    from tests import planned_shapes as ps
    res = {"plan_blocks": os.environ.get("GKLHIP_PLAN_BLOCKS", "")}
    with native.PairHmmContext(fma_mode=a.fma) as host, native.PairHmmContext(fma_mode=a.fma, finalize=native.FINALIZE_DEVICE_F64) as dev:
        for name in a.names.split(","):
            b = ps.batch(name)
            out = host.compute(b)
            h = ps.digests(out, *host.raw(b.n_pairs))
            d_out = dev.compute_device(native.DeviceBatch.upload(b))
            torch.cuda.synchronize()
            res[name] = {"host": h, "device": ps.digests(d_out.cpu().numpy(), *dev.raw(b.n_pairs))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
