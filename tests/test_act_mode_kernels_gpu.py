"""GPU: bd_tanh_normal_mode (csrc/act.hip: tanh_normal_mode_index, one wave per row) against the float64 selection
reference tests/act_mode_ref.py -- the returned index admissible, the action that index' float64 action, planted exact ties
broken towards the first draw, in-kernel Philox draws equal to a run fed bd_rng_fill's buffer.  The input conditions of
every case are asserted on the float64 side by tests/test_act_mode_ref_cpu.py."""
import ctypes as C

import pytest
import torch

from tests import act_mode_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-5          # the acting step's tolerance (tests/test_act_step_gpu.py)
CASES = [(N, A, n, kind) for (N, A, n) in R.SIZES for kind in R.kinds_of(A)]


def run_mode(mean, sd, eps, n=None, seed=0, step=0, stream_id=0, want_index=True):
    """bd_tanh_normal_mode on CPU tensors (eps None: in-kernel draws, n of them) -> (action, index) on the host."""
    from big_dreamer_amd import _cabi as cabi
    N, A = mean.shape
    m, s = mean.cuda().contiguous(), sd.cuda().contiguous()
    e = None if eps is None else eps.cuda().contiguous()
    n = eps.shape[0] if eps is not None else n
    action = torch.full((N, A), float("nan"), device="cuda")
    index = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    cabi.check(cabi.lib.bd_tanh_normal_mode(m.data_ptr(), s.data_ptr(), None if e is None else e.data_ptr(), seed, step,
                                            stream_id, N, A, n, action.data_ptr(), index.data_ptr() if want_index else None,
                                            cabi.stream()))
    torch.cuda.synchronize()
    return action.cpu(), index.cpu()


@pytest.mark.parametrize("N, A, n, kind", CASES)
def test_index_is_admissible_and_the_action_is_its_draw(N, A, n, kind):
    mean, sd, eps = R.make_case(N, A, n, kind)
    action, index = run_mode(mean, sd, eps)
    multi = R.check(index, action, mean, sd, eps, TOL, tag=f"N={N} A={A} n={n} {kind}: ")
    print(f"N={N} A={A} n={n} {kind}: {multi} of {N} rows with more than one admissible index")
    assert multi <= R.MULTI_CAP * N
    single = R.admissible(mean, sd, eps).sum(0) == 1
    assert torch.equal(index.long()[single], R.winner(mean, sd, eps)[single])
    # index = NULL is allowed and changes nothing
    action2, untouched = run_mode(mean, sd, eps, want_index=False)
    assert torch.equal(action2, action) and bool((untouched == -1).all())


@pytest.mark.parametrize("N, A, n, kind", [c for c in CASES if c[2] in R.TIES])
def test_exact_ties_go_to_the_first_draw(N, A, n, kind):
    mean, sd, eps0 = R.make_case(N, A, n, kind)
    for j1, j2 in R.TIES[n]:
        eps = R.plant_tie(mean, sd, eps0, j1, j2)
        action, index = run_mode(mean, sd, eps)
        R.check(index, action, mean, sd, eps, TOL, tag=f"tie ({j1}, {j2}) N={N} A={A} n={n} {kind}: ")
        only = R.admissible(mean, sd, eps).sum(0) == 2          # j1 and j2 and nothing else
        print(f"tie ({j1}, {j2}) N={N} A={A} n={n} {kind}: {int((~only).sum())} of {N} rows admit a third index")
        assert not bool((index == j2).any()), f"tie ({j1}, {j2}): the later of two identical draws was returned"
        assert bool((index.long()[only] == j1).all()), f"tie ({j1}, {j2}): {index.tolist()}"


@pytest.mark.parametrize("N, A, n", [(1, 2, 1), (17, 3, 65), (70, 17, 100), (5, 1, 100), (3, 64, 7)])
def test_in_kernel_noise_is_the_rng_fill_stream(N, A, n):
    """eps_mode = NULL: element i of the (n, N, A) draws is what bd_rng_fill(BD_RNG_NORMAL, seed, step, stream) writes at i."""
    from big_dreamer_amd import _cabi as cabi
    mean, sd = torch.linspace(-0.9, 0.9, N * A).view(N, A).contiguous(), torch.full((N, A), 0.5)
    seed, step, stream_id = 0x1234_5678_9ABC_DEF0, 41, 11
    buf = torch.zeros(n, N, A, device="cuda")
    r = cabi.RngFillArgs()
    r.n, r.seed, r.step = 1, seed, step
    r.t[0] = cabi.RngTensor(buf.data_ptr(), buf.numel(), cabi.BD_RNG_NORMAL, stream_id)
    cabi.check(cabi.lib.bd_rng_fill(C.byref(r), cabi.stream()))
    fed = run_mode(mean, sd, buf.cpu())
    own = run_mode(mean, sd, None, n=n, seed=seed, step=step, stream_id=stream_id)
    assert torch.equal(fed[1], own[1]) and torch.equal(fed[0], own[0])
    other = run_mode(mean, sd, None, n=n, seed=seed, step=step + 1, stream_id=stream_id)
    assert not torch.equal(other[0], own[0]), "another decision counter gave the same draws"
