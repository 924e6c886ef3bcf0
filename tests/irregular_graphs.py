"""Hand-made graph topologies for the camera+LiDAR+radar tests (test infrastructure).

The synthetic windows (batch3dmot_amd.synth) give every destination at most k in-edges and every source a few dozen out-edges.
The shapes here are the ones the `past` run sums of the edge kernels (b3d_estream.hpp run_sums: per destination inside aligned
16-edge blocks), the run-tail lists of the graph build (b3d_prep.hip graph_past_lists) and the three-way split of a source's
`future` list (b3d_node.hpp) have to get right.  "Block": an aligned 16-edge block of the edge order; "tile": a 64-row tile of
the edge kernels.

Every builder returns (N, edge_index [2, E] int64); the edges are grouped by ascending destination unless the name says otherwise.
"""
import torch

BLOCK = 16


def grouped(ei):
    """Stable sort by destination: the order the graph build recognises as grouped (dst_unsorted = 0)."""
    return ei[:, torch.argsort(ei[1], stable=True)].contiguous()


def shuffled(ei, seed):
    perm = torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(seed))
    return ei[:, perm].contiguous()


def reversed_order(ei):
    return torch.flip(ei, dims=[1]).contiguous()


def block_runs():
    """T1: runs that line up with the blocks and runs that start at many offsets inside one.  Destination 2 has in-degree 16 from
    edge 0 (one key fills a whole block: all four scan steps carry); then 15, 17, 1, 31, 32, 33 (three blocks), 3, 48, 5, 64 (five
    blocks, across the tile boundary at 256), 2, 7.  E = 274 ends inside a block."""
    n = 60
    degrees = [16, 15, 17, 1, 31, 32, 33, 3, 48, 5, 64, 2, 7]
    dsts = [2, 3, 5, 6, 9, 10, 14, 20, 21, 30, 31, 44, 59]          # ascending, with nodes that receive nothing in between
    g = torch.Generator().manual_seed(101)
    dst = torch.cat([torch.full((d,), v, dtype=torch.long) for d, v in zip(degrees, dsts)])
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    return n, torch.stack([src, dst]).contiguous()


def long_run(n=400, hub=150, hub_in=300, rest=500, seed=102):
    """T2: one destination with 300 in-edges (19+ blocks over 5+ tiles: several workgroups write tails of the same node) among
    ~500 random edges."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (hub_in + rest,), generator=g)
    dst = torch.randint(0, n - 1, (rest,), generator=g)
    dst = torch.cat([torch.full((hub_in,), hub, dtype=torch.long), dst + (dst >= hub).long()])     # the others avoid the hub
    return n, grouped(torch.stack([src, dst]))


def out_hub(n=320, seed=103):
    """T3: source 5 with 250 out-edges; sources 300 .. 303 with out-degree 1, 2, 3 and 4 (the node kernel's three parts of a
    source's `future` list, beg + len * part / 3: some parts empty); 150 random edges among the nodes below 300."""
    g = torch.Generator().manual_seed(seed)
    src = [torch.full((250,), 5, dtype=torch.long)]
    dst = [torch.arange(10, 260)]
    for i, deg in enumerate((1, 2, 3, 4)):
        src.append(torch.full((deg,), 300 + i, dtype=torch.long))
        dst.append(torch.randint(0, n, (deg,), generator=g))
    r_src = torch.randint(0, 299, (150,), generator=g)
    src.append(r_src + (r_src >= 5).long())                          # the hub's out-degree stays 250
    dst.append(torch.randint(0, n, (150,), generator=g))
    return n, grouped(torch.stack([torch.cat(src), torch.cat(dst)]))


def degenerate():
    """T4: node 0 and 14 .. 19 isolated, 1 and 2 sources only, 7 a sink only, the edge (1 -> 7) three times, two self loops."""
    src = torch.tensor([1, 1, 1, 2, 3, 4, 5, 5, 6, 9, 10, 12, 20, 21, 22, 4, 9])
    dst = torch.tensor([7, 7, 7, 7, 4, 5, 6, 8, 8, 11, 11, 13, 21, 22, 20, 4, 9])
    return 23, grouped(torch.stack([src, dst]))


TINY = [(1, 1), (2, 1), (3, 15), (17, 16), (16, 17), (20, 64), (16, 129)]


def tiny(n, e):
    """T5: N nodes, E random edges grouped by destination."""
    g = torch.Generator().manual_seed(n * 1000 + e)
    return n, torch.stack([torch.randint(0, n, (e,), generator=g), torch.sort(torch.randint(0, n, (e,), generator=g)).values])


def one_sink(n=40, e=200, sink=7):
    """T6: every edge into one node."""
    g = torch.Generator().manual_seed(106)
    return n, torch.stack([torch.randint(0, n, (e,), generator=g), torch.full((e,), sink, dtype=torch.long)])


def straddling_pair():
    """T8 parts: graph A (30 nodes, 42 edges = 2 blocks + 10) and graph B (36 nodes) whose first destination has 12 in-edges --
    collated, B's first run covers batch edges 42 .. 53 across the block boundary at 48."""
    g = torch.Generator().manual_seed(108)
    n_a, ei_a = 30, grouped(torch.stack([torch.randint(0, 30, (42,), generator=g), torch.randint(0, 30, (42,), generator=g)]))
    dst_b = torch.cat([torch.zeros(12, dtype=torch.long), torch.randint(1, 36, (70,), generator=g)])
    ei_b = grouped(torch.stack([torch.randint(0, 36, (82,), generator=g), dst_b]))
    assert int(ei_b[1][:13].eq(0).sum()) == 12
    return (n_a, ei_a), (36, ei_b)


def run_tails(ei, n):
    """The run-tail lists of a graph grouped by destination, restated: for every node, the last edge of each of its
    (node, aligned 16-edge block) runs.  Returns (past_ptr [N + 1], past_rows) as lists."""
    dst = ei[1].tolist()
    ptr, rows = [0], []
    by_node = [[] for _ in range(n)]
    for i, d in enumerate(dst):
        by_node[d].append(i)
    for node in range(n):
        edges = by_node[node]
        assert not edges or edges[-1] - edges[0] + 1 == len(edges), "not grouped by destination"
        blocks = sorted({i // BLOCK for i in edges})
        rows += [max(i for i in edges if i // BLOCK == b) for b in blocks]
        ptr.append(len(rows))
    return ptr, rows


def clr_data(n, edge_index, seed):
    """A window with the hand-made edges: node features (pose, camera, LiDAR, radar, timestamps) of the first n detections of a
    synthetic window, a seeded float64 edge_attr [E, 4]."""
    from batch3dmot_amd import synth
    from batch3dmot_amd.data import Data
    base = synth.make_graph(max(n, 40) + 5, None, k=3, graph_idx=2000 + seed, modalities=True)
    assert base.pose_feats.size(0) >= n
    e = edge_index.size(1)
    g = torch.Generator().manual_seed(seed)
    return Data(pose_feats=base.pose_feats[:n].clone(), img_feats=base.img_feats[:n].clone(),
                lidar_feats=base.lidar_feats[:n].clone(), radar_feats=base.radar_feats[:n].clone(),
                node_timestamps=base.node_timestamps[:n].clone(), edge_index=edge_index.contiguous(),
                edge_attr=torch.randn(e, 4, generator=g, dtype=torch.float64))


EDGE_STACKS = ("edge_encoder", "att_edge_encoder", "message_passing", "edge_classifier")


def defuse_edge_ties(ora64, data, margin=1e-5, seed=0, passes=40):
    """In place: nudge rows of data.edge_attr until no ReLU pre-activation of the edge-side stacks of the float64 oracle `ora64` is
    within `margin` of zero (as test_mp_layer_hip._defuse_relu_ties does for one layer).  Such a unit may take the other branch in
    a correct fp32 evaluation; on graphs of a few dozen edges the flip of one moves a whole edge's share of a weight gradient -- past
    the escape clause of conftest.assert_grad_close, which is sized for a few hundred edges.  A per-edge unit moves its own edge,
    a per-node unit of the message passing the edges at its node.  Returns the number of passes that nudged."""
    names = {m: n for n, m in ora64.named_modules()}
    ei = data.edge_index
    e, n = ei.size(1), data.pose_feats.size(0)
    bad = torch.zeros(e, dtype=torch.bool)

    def hook(mod, _i, out):
        if out.numel() == 0:
            return
        close = out.detach().abs().min(dim=1).values < margin
        if out.size(0) == e:
            bad.__ior__(close)
        elif out.size(0) == n:
            nodes = torch.nonzero(close).squeeze(1)
            bad.__ior__(torch.isin(ei[0], nodes) | torch.isin(ei[1], nodes))

    hooks = []
    for seq in ora64.modules():
        if isinstance(seq, torch.nn.Sequential) and names[seq].split(".")[0] in EDGE_STACKS:
            ch = list(seq)
            for a, b in zip(ch, ch[1:]):
                if isinstance(a, torch.nn.Linear) and isinstance(b, torch.nn.ReLU):
                    hooks.append(a.register_forward_hook(hook))
    g = torch.Generator().manual_seed(seed)
    d64 = data.__class__(**{k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in data.__dict__.items()})
    try:
        for it in range(passes):
            bad.zero_()
            d64.edge_attr = data.edge_attr.double()
            with torch.no_grad():
                ora64(d64)
            if not bad.any():
                return it
            data.edge_attr[bad] += 0.05 * torch.randn(int(bad.sum()), data.edge_attr.size(1), generator=g, dtype=data.edge_attr.dtype)
    finally:
        for h in hooks:
            h.remove()
    raise AssertionError("could not move the ReLU pre-activations of the edge stacks away from zero")
