"""Worker of tests/test_replica_cpu.py: one gloo rank.  DataParallel.agree and broadcast_ on CPU tensors: equal vectors
agree; one rank differing in one position -- positions holding INT64_MIN and -1 included -- gives the same per-position
verdict on every rank; broadcast_ makes every rank equal to src, for src 0 and 1."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd.parallel import DataParallel  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def gathered(x):
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, x)
    return out


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dp = DataParallel(world, rank)
    base = [I64_MIN, -1, 0, 1, I64_MAX, 0x123456789ABCDEF, -0x123456789ABCDEF, I64_MIN + 1, -2, 42]
    n = len(base)

    # equal vectors agree; the input is left alone
    w = torch.tensor(base, dtype=torch.int64)
    v = dp.agree(w)
    assert v.dtype == torch.bool and v.shape == (n,) and bool(v.all()), v
    assert w.tolist() == base
    hi, lo = dp.max_min_(w)
    assert hi.tolist() == base and lo.tolist() == base

    # one rank differs in one position: every differing rank, every position, a change up and a change down
    for who in range(world):
        for pos in range(n):
            for new in (base[pos] ^ 1, base[pos] ^ I64_MIN, ~base[pos]):
                w = torch.tensor(base, dtype=torch.int64)
                if rank == who:
                    w[pos] = new
                v = dp.agree(w).tolist()
                assert v == [i != pos for i in range(n)], (who, pos, new, v)
                hi, lo = dp.max_min_(w)
                assert hi[pos].item() == max(base[pos], new) and lo[pos].item() == min(base[pos], new), (who, pos, new)
                assert all(x == v for x in gathered(v))

    # all ranks different everywhere: nothing agrees, max and min are the true ones
    w = torch.tensor([b ^ (rank + 1) for b in base], dtype=torch.int64)
    hi, lo = dp.max_min_(w)
    assert not bool(dp.agree(w).any())
    for i, b in enumerate(base):
        vals = [b ^ (r + 1) for r in range(world)]
        assert hi[i].item() == max(vals) and lo[i].item() == min(vals)

    # broadcast_: every rank equal to src
    for src in (0, 1):
        f = torch.arange(7, dtype=torch.float32) * (rank + 1) + rank
        f[3] = float("nan") if rank == src else 0.0
        want = torch.arange(7, dtype=torch.float32) * (src + 1) + src
        want[3] = float("nan")
        out = dp.broadcast_(f, src)
        assert out is f and f.view(torch.int32).tolist() == want.view(torch.int32).tolist(), (src, f)
        i = dp.broadcast_(torch.tensor([rank, I64_MIN + rank], dtype=torch.int64), src)
        assert i.tolist() == [src, I64_MIN + src]

    dist.barrier()
    if rank == 0:
        print(f"REPLICA_CPU_OK world={world}")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
