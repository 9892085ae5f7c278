"""Records tests/golden/sharded_exchange_plan.npz: the exchange plan of ShardedStreamRunner._exchange_plan (torch plan, no device)
for every rank of worlds of 2 and 3 on the stream tests/test_sharded.py::test_targeted_relabelling_gloo uses, from a checkout of
the commit whose behaviour is to be kept:

    python tests/golden/make_sharded_plan.py /path/to/that/checkout

The fields are stored under the names of the finished plan (tests/test_sharded_phases.py); a checkout from before the plan had one
spelling is read by its second one (scnt, rcnt, sstart_)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_sharded_phases as T  # noqa: E402

OLD_NAMES = {"send_cnt": "scnt", "recv_cnt": "rcnt", "sstart": "sstart_"}


def main():
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from tpnet_amd.sharded import ShardedStreamRunner
    out = {}
    for world, rank in T.PLAN_RANKS:
        R, _ = T.exchange_plan_of(ShardedStreamRunner, world, rank)
        for f in T.PLAN_FIELDS:
            v = R[OLD_NAMES[f]] if OLD_NAMES.get(f) in R else R[f]
            out[f"w{world}_r{rank}_{f}"] = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(HERE, "sharded_exchange_plan.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
