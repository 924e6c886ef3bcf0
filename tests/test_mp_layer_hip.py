"""GPU: CausalMessagePassing.forward as a standalone operator against the oracle's restatement of
pose_gnn.py:125-252 / clr_att_gnn.py:227-356 (the oracle itself is pinned to the reference by the
per-layer captures of tests/golden/g1_pose.pt and g2_clr.pt)."""
import pytest
import torch

from oracle import ref_torch
from oracle.seeded import seeded_fill_

pytestmark = pytest.mark.gpu


def _graph(n, k, seed):
    from batch3dmot_amd import synth
    return synth.make_graph(n, None, k=k, graph_idx=seed)


def _defuse_relu_ties(ora, x, x0, e, edge_index, gen, margin=1e-4, att=None):
    """Random inputs put ~1 in 10^7 ReLU pre-activations within fp32 rounding of zero; such a unit may
    switch between two correct fp32 evaluations and move the gradients of its row by O(1).  Nudge the
    edge features of the affected rows (float64 probe of every Linear that feeds a ReLU) until every
    pre-activation is at least `margin` away from zero, so that the comparison below can be tight."""
    import copy
    o64 = copy.deepcopy(ora).double()
    pre = []
    hooks = []
    for seq in (o64.edge_update, o64.create_past_msgs, o64.create_future_msgs, o64.combine_future_past):
        mods = list(seq)
        for a, b in zip(mods, mods[1:]):
            if isinstance(a, torch.nn.Linear) and isinstance(b, torch.nn.ReLU):
                hooks.append(a.register_forward_hook(lambda _m, _i, out: pre.append(out.detach())))
    e = e.clone()
    n = x.size(0)
    for _ in range(60):
        pre.clear()
        with torch.no_grad():
            if att is None:
                o64(x.double(), edge_index, e.double(), x0.double())
            else:
                o64(x.double(), edge_index, e.double(), x0.double(), att.double())
        bad_edges = torch.zeros(e.size(0), dtype=torch.bool)
        for t in pre:
            close = t.abs().min(dim=1).values < margin
            if t.size(0) == e.size(0):
                bad_edges |= close
            else:                                   # node-level unit: move the messages that reach the node
                assert t.size(0) == n
                bad_edges |= close[edge_index[1]]
        if not bad_edges.any():
            break
        e[bad_edges] += 0.05 * torch.randn(int(bad_edges.sum()), e.size(1), generator=gen)
    else:
        raise AssertionError("could not move the ReLU pre-activations away from zero")
    for h in hooks:
        h.remove()
    return e


@pytest.mark.parametrize("n,k", [(90, 6), (700, 12), (3000, 13)])
def test_pose_layer_forward_backward_match_oracle(n, k):
    from batch3dmot_amd.pose_gnn import CausalMessagePassing
    dev = torch.device("cuda:0")
    d = _graph(n, k, 31)
    ora = ref_torch.CausalMessagePassing("p")
    seeded_fill_(ora, 5)
    m = CausalMessagePassing()
    m.load_state_dict(ora.state_dict())
    m.to(dev)
    g = torch.Generator().manual_seed(1)
    N, E = d.pose_feats.size(0), d.edge_index.size(1)
    x = torch.randn(N, 48, generator=g)
    x0 = torch.randn(N, 48, generator=g)
    e = torch.randn(E, 32, generator=g)
    cx, ce = torch.randn(N, 48, generator=g), torch.randn(E, 32, generator=g)

    e = _defuse_relu_ties(ora, x, x0, e, d.edge_index, g, margin=1e-4 if n < 3000 else 3e-5)

    def run(mod, dev_):
        xs = [t.clone().to(dev_).requires_grad_(True) for t in (x, x0, e)]
        xn, en = mod(xs[0], d.edge_index.to(dev_), xs[2], xs[1])
        ((xn * cx.to(dev_)).sum() + (en * ce.to(dev_)).sum()).backward()
        return xn.detach().cpu(), en.detach().cpu(), [t.grad.cpu() for t in xs], \
            {k_: p.grad.cpu() for k_, p in mod.named_parameters()}

    ref = run(ora, torch.device("cpu"))
    got = run(m, dev)
    torch.testing.assert_close(got[0], ref[0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(got[1], ref[1], rtol=1e-4, atol=1e-5)
    for a, b, name in zip(got[2], ref[2], ("d x", "d initial_x", "d edge_attr")):
        scale = b.abs().max().item()
        assert (a - b).abs().max().item() <= 1e-4 * scale + 1e-6, name
    for k_ in ref[3]:
        scale = ref[3][k_].abs().max().item()
        assert (got[3][k_] - ref[3][k_]).abs().max().item() <= 1e-4 * scale + 1e-6, k_


def test_pose_layer_only_node_output_gradient():
    """d e' absent (None): treated as zero."""
    from batch3dmot_amd.pose_gnn import CausalMessagePassing
    dev = torch.device("cuda:0")
    d = _graph(120, 5, 77)
    ora = ref_torch.CausalMessagePassing("p")
    seeded_fill_(ora, 6)
    m = CausalMessagePassing()
    m.load_state_dict(ora.state_dict())
    m.to(dev)
    g = torch.Generator().manual_seed(2)
    N, E = d.pose_feats.size(0), d.edge_index.size(1)
    x, x0, e = torch.randn(N, 48, generator=g), torch.randn(N, 48, generator=g), torch.randn(E, 32, generator=g)
    e = _defuse_relu_ties(ora, x, x0, e, d.edge_index, g)
    xr = x.clone().requires_grad_(True)
    ora(xr, d.edge_index, e, x0)[0].sum().backward()
    xg = x.clone().to(dev).requires_grad_(True)
    m(xg, d.edge_index.to(dev), e.to(dev), x0.to(dev))[0].sum().backward()
    scale = xr.grad.abs().max().item()
    assert (xg.grad.cpu() - xr.grad).abs().max().item() <= 1e-4 * scale


@pytest.mark.parametrize("n,k", [(150, 7), (600, 10), (3000, 13)])
def test_clr_layer_forward_backward_match_oracle(n, k):
    """clr_att_gnn.py:227-356 as an operator of its own: outputs, the gradients of all five inputs (x, initial_x,
    edge_attr, att_edge_attr) and of the ten Linear layers against the CPU oracle, every entry at 1e-4 on inputs whose
    ReLU pre-activations all stay clear of zero (data-dependent masks, up to the benchmark's 3,000 nodes / ~31,000 edges)."""
    d = _graph(n, k, 13)
    _clr_layer_against_oracle(d.pose_feats.size(0), d.edge_index, margin=1e-4 if n < 3000 else 3e-5)


@pytest.mark.parametrize("topo", ["t1", "t2", "t3", "t7_t1_shuffled", "t7_t1_reversed", "t7_t2_shuffled", "t7_t2_reversed"])
def test_clr_layer_irregular_topologies(topo):
    """The same flow on the hand-made graphs of tests/irregular_graphs.py: T1 (runs that fill a whole 16-edge block or start at
    many offsets inside one, up to five blocks per run), T2 (a destination with 300 in-edges: 19+ blocks over 5+ tiles), T3 (a
    source with 250 out-edges, sources with out-degree 1 .. 4) and T7 (T1 and T2 out of destination order).  A wrong per-node sum of
    the `past` runs or of the three parts of a `future` list shows in x' directly."""
    import irregular_graphs as ig
    base = {"t1": ig.block_runs, "t2": ig.long_run, "t3": ig.out_hub}
    name = topo.split("_")[-2] if topo.startswith("t7") else topo
    n, ei = base[name]()
    if topo.endswith("shuffled"):
        ei = ig.shuffled(ei, 7)
    elif topo.endswith("reversed"):
        ei = ig.reversed_order(ei)
    _clr_layer_against_oracle(n, ei)


def _clr_layer_against_oracle(N, edge_index, margin=1e-4):
    from batch3dmot_amd.clr_att_gnn import CausalMessagePassing
    dev = torch.device("cuda:0")
    ora = ref_torch.CausalMessagePassing("clr")
    seeded_fill_(ora, 8)
    m = CausalMessagePassing()
    m.load_state_dict(ora.state_dict())
    m.to(dev)
    g = torch.Generator().manual_seed(3)
    E = edge_index.size(1)
    x, x0 = torch.randn(N, 96, generator=g), torch.randn(N, 96, generator=g)
    e, att = torch.randn(E, 64, generator=g), torch.randn(E, 64, generator=g)
    cx, ce = torch.randn(N, 96, generator=g), torch.randn(E, 64, generator=g)
    e = _defuse_relu_ties(ora, x, x0, e, edge_index, g, margin=margin, att=att)
    with torch.no_grad():
        rx, re = ora(x, edge_index, e, x0, att)
        gx, ge = m(x.to(dev), edge_index.to(dev), e.to(dev), x0.to(dev), att.to(dev))
    torch.testing.assert_close(gx.cpu(), rx, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ge.cpu(), re, rtol=1e-4, atol=1e-4)

    def run(mod, dev_):
        xs = [t.clone().to(dev_).requires_grad_(True) for t in (x, x0, e, att)]
        xn, en = mod(xs[0], edge_index.to(dev_), xs[2], xs[1], xs[3])
        ((xn * cx.to(dev_)).sum() + (en * ce.to(dev_)).sum()).backward()
        return [t.grad.cpu() for t in xs], {k_: p.grad.cpu() for k_, p in mod.named_parameters()}

    ref_in, ref_w = run(ora, torch.device("cpu"))
    got_in, got_w = run(m, dev)
    for a, b, name in zip(got_in, ref_in, ("d x", "d initial_x", "d edge_attr", "d att_edge_attr")):
        assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item() + 1e-6, name
    for k_ in ref_w:
        assert (got_w[k_] - ref_w[k_]).abs().max().item() <= 1e-4 * ref_w[k_].abs().max().item() + 1e-6, k_
    m.zero_grad()
    with torch.no_grad():                                         # inference forwards keep no state
        out = m(x.to(dev), edge_index.to(dev), e.to(dev), x0.to(dev), att.to(dev))
    assert not out[0].requires_grad


@pytest.mark.parametrize("kind", ["p", "clr"])
def test_dead_relu_units_carry_no_gradient(kind):
    """The backward sweep reads ReLU BIT MASKS written by the forward (one bit per saved hidden value, b3d_dev.hpp) instead of the
    activations: a unit whose pre-activation is EXACTLY zero (dead rows of the Linear in front of the ReLU, here at both ends and
    across the 32-value word boundaries of every masked tensor) must pass no gradient, as torch's relu' does; everything else as the
    oracle."""
    from conftest import assert_grad_close
    dev = torch.device("cuda:0")
    d = _graph(220, 8, 23)
    ora = ref_torch.CausalMessagePassing(kind)
    seeded_fill_(ora, 12)
    dead = {}
    with torch.no_grad():
        for name, seq in (("edge_update", ora.edge_update), ("create_past_msgs", ora.create_past_msgs),
                          ("create_future_msgs", ora.create_future_msgs)):
            lins = [mod for mod in seq if isinstance(mod, torch.nn.Linear)]
            for li, lin in enumerate(lins[:-1]):                       # every Linear that feeds a ReLU
                n_out = lin.out_features
                rows = sorted({0, 1, 7, 8, 31, 32, 33, n_out // 2, n_out - 2, n_out - 1} & set(range(n_out)))
                lin.weight[rows] = 0.0
                lin.bias[rows] = 0.0
                dead[f"{name}.{2 * li}"] = rows
    if kind == "p":
        from batch3dmot_amd.pose_gnn import CausalMessagePassing
        dx, de = 48, 32
    else:
        from batch3dmot_amd.clr_att_gnn import CausalMessagePassing
        dx, de = 96, 64
    m = CausalMessagePassing()
    m.load_state_dict(ora.state_dict())
    m.to(dev)
    g = torch.Generator().manual_seed(5)
    N, E = d.pose_feats.size(0), d.edge_index.size(1)
    x, x0, e = torch.randn(N, dx, generator=g), torch.randn(N, dx, generator=g), torch.randn(E, de, generator=g)
    att = torch.randn(E, 64, generator=g) if kind == "clr" else None
    cx, ce = torch.randn(N, dx, generator=g), torch.randn(E, de, generator=g)

    def run(mod, dev_):
        xs = [t.clone().to(dev_).requires_grad_(True) for t in (x, x0, e)]
        extra = (att.clone().to(dev_),) if att is not None else ()
        xn, en = mod(xs[0], d.edge_index.to(dev_), xs[2], xs[1], *extra)
        ((xn * cx.to(dev_)).sum() + (en * ce.to(dev_)).sum()).backward()
        return [t.grad.cpu() for t in xs], {k_: p.grad.cpu() for k_, p in mod.named_parameters()}

    ref_in, ref_w = run(ora, torch.device("cpu"))
    got_in, got_w = run(m, dev)
    for key, rows in dead.items():
        assert float(ref_w[key + ".weight"][rows].abs().max()) == 0.0           # the oracle agrees that they are dead
        assert float(got_w[key + ".weight"][rows].abs().max()) == 0.0, key
        assert float(got_w[key + ".bias"][rows].abs().max()) == 0.0, key
    for a, b, name in zip(got_in, ref_in, ("d x", "d initial_x", "d edge_attr")):
        assert_grad_close(a, b, name)
    for k_ in ref_w:
        assert_grad_close(got_w[k_], ref_w[k_], k_)


@pytest.mark.parametrize("kind", ["p", "clr"])
@pytest.mark.parametrize("case", ["inf", "nan", "huge", "denormal", "mixed"])
def test_non_finite_and_extreme_inputs(kind, case):
    """Edge values through the bf16x6 layers (three-way bf16 split of every operand, six piece products).

    Finite extremes -- 3e38 (the split's residuals stay finite) and denormals -- give the reference's values.  A NaN
    spreads exactly as in the reference: the Linear layers propagate it through every product and ReLU keeps it
    (b3d_common.hpp relu1).  +-inf: the split computes x - hi(x) = inf - inf, so the FIRST Linear that sees an infinite
    operand already returns NaN where the reference's returns +-inf and turns NaN one Linear later (rows of both signs
    meet); every stack here has at least two Linears, so the rows that come out non-finite are the same rows, which is
    what is asserted (element by element inside them the reference may hold +-inf or 0 = relu(-inf) where the kernels
    hold NaN)."""
    from batch3dmot_amd import clr_att_gnn, pose_gnn
    dev = torch.device("cuda:0")
    d = _graph(150, 7, 47)
    ora = ref_torch.CausalMessagePassing(kind)
    seeded_fill_(ora, 12)
    m = (pose_gnn if kind == "p" else clr_att_gnn).CausalMessagePassing()
    m.load_state_dict(ora.state_dict())
    m.to(dev)
    dx, de = (48, 32) if kind == "p" else (96, 64)
    g = torch.Generator().manual_seed(9)
    N, E = d.pose_feats.size(0), d.edge_index.size(1)
    x, x0, e = torch.randn(N, dx, generator=g), torch.randn(N, dx, generator=g), torch.randn(E, de, generator=g)
    att = torch.randn(E, 64, generator=g) if kind == "clr" else None
    if case == "inf":
        x[5, 3] = float("inf")
        e[7, 2] = float("-inf")
    elif case == "nan":
        e[11, 0] = float("nan")
        x0[9, 1] = float("nan")
    elif case == "huge":
        x[5, 3] = 3e38
        e[7, 2] = -3e38
    elif case == "mixed":                                   # magnitudes 1e-20 .. 1e20 inside one row, alternating signs
        mags = 10.0 ** torch.linspace(-20, 20, de)
        e[7] = mags * torch.tensor([1.0, -1.0]).repeat(de // 2)
        x[5, : dx // 2] = (10.0 ** torch.linspace(-15, 15, dx // 2))
    else:
        e[7] = 1e-40
        x[5, :8] = -3e-39
    args = (x, d.edge_index, e, x0) + ((att,) if att is not None else ())
    with torch.no_grad():
        rx, re = ora(*args)
        gx, ge = m(*[t.to(dev) for t in args])
    gx, ge = gx.cpu(), ge.cpu()
    for have, want, name in ((gx, rx, "x'"), (ge, re, "e'")):
        bad_w = ~torch.isfinite(want).all(1)
        bad_h = ~torch.isfinite(have).all(1)
        assert torch.equal(bad_w, bad_h), (name, int(bad_w.sum()), int(bad_h.sum()))
        assert bool(torch.isnan(have[bad_h]).any(1).all())          # a non-finite row never looks finite in part only
        if case in ("inf", "nan"):
            assert int(bad_w.sum()) > 0
        else:
            assert int(bad_w.sum()) == 0
        ok = ~bad_w
        scale = want[ok].abs().max(1, keepdim=True).values.clamp_min(1e-6)   # per row: the huge rows do not hide the others
        assert float(((have[ok] - want[ok]).abs() / scale).max()) < 1e-4, name


def test_layer_builds_the_graph_structure_once_per_edge_index_tensor():
    """Repeated applications to the same edge_index tensor (a model's gnn_depth iterations) share one CSR / CSC build and
    one endpoint validation; an in-place edit of the tensor, or another tensor, rebuilds."""
    from batch3dmot_amd import mp_layer
    from batch3dmot_amd.pose_gnn import CausalMessagePassing
    dev = torch.device("cuda:0")
    d = _graph(60, 5, 3)
    m = CausalMessagePassing().to(dev)
    g = torch.Generator().manual_seed(4)
    N, E = d.pose_feats.size(0), d.edge_index.size(1)
    x, x0, e = (torch.randn(N, 48, generator=g).to(dev), torch.randn(N, 48, generator=g).to(dev), torch.randn(E, 32, generator=g).to(dev))
    ei = d.edge_index.to(dev)
    with torch.no_grad():
        a = m(x, ei, e, x0)
        g1 = mp_layer._GRAPH_CACHE[id(m)][2]
        b = m(x, ei, e, x0)
        assert mp_layer._GRAPH_CACHE[id(m)][2] is g1 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ei[0, 0] = ei[0, 1]                       # in place: the version counter moves
        m(x, ei, e, x0)
        assert mp_layer._GRAPH_CACHE[id(m)][2] is not g1
        g2 = mp_layer._GRAPH_CACHE[id(m)][2]
        m(x, ei.clone(), e, x0)
        assert mp_layer._GRAPH_CACHE[id(m)][2] is not g2
        bad = ei.clone()
        bad[1, 3] = N + 7
        with pytest.raises(ValueError):
            m(x, bad, e, x0)

    # the cache lives outside the module (a _lib.Graph holds ctypes pointers): a layer that has run can be copied and
    # pickled, a structure built on one stream is usable from another, and the entry dies with the module
    import copy, gc, pickle
    with torch.no_grad():
        want = m(x, ei, e, x0)
        m2 = copy.deepcopy(m)
        pickle.dumps(m)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = m(x, ei, e, x0)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        got2 = m2(x, ei, e, x0)
        assert torch.equal(got2[0], want[0])
    key = id(m)
    del m, got, want
    gc.collect()
    assert key not in mp_layer._GRAPH_CACHE
