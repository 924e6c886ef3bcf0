"""Drop-in for the reference's ``batch_3dmot.models.clr_att_gnn`` (GNN, CausalMessagePassing).

Same constructor signature, ``forward(data)`` contract and ``state_dict`` keys as
``/root/reference/batch_3dmot/models/clr_att_gnn.py:16-356``.  The three frozen encoder modules
are called as the reference calls them (``resnet.encode``, ``pointnet.forward_feat``,
``radarnet.forward_feat``; they are adjacent to the hot path and stay on PyTorch-ROCm);
everything downstream -- modality heads, the cross-edge modality attention, att_edge_encoder, the
encoders, 6 message-passing layers and the sigmoid classifier, forward and backward -- runs in
the HIP kernels of ``libb3d_hip.so``.

The cross-edge attention calls ``nn.MultiheadAttention`` with ONE query and ONE key per edge
(clr_att_gnn.py:144-155): the softmax over a single key is 1, so every call equals
``out_proj(v_proj(value))`` exactly and the query / key projections are dead.  The kernels
evaluate that affine map once per node and gather it per edge; the ``nn.MultiheadAttention``
modules are kept as parameter holders so that checkpoints load unchanged.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch
from torch import nn

from . import _lib
from ._lib import (B3D_FLAG_DEFER_SIDE_JOIN, B3D_FLAG_RUN_DEAD_KNN, B3D_FLAG_SINGLE_STREAM, B3D_FLAG_SKIP_DEAD_LAST_MESSAGES,
                   B3D_FLAG_TRAINING)
from .pose_gnn import GATConvParams, _linears, _mlp


class CausalMessagePassing(nn.Module):
    """Parameters of reference clr_att_gnn.py:193-222 (aggr='add')."""

    def __init__(self):
        super().__init__()
        self.edge_update = _mlp([320, 256, 128, 64])
        self.create_past_msgs = _mlp([256, 192, 128])
        self.create_future_msgs = _mlp([256, 192, 128])
        self.combine_future_past = _mlp([256, 192, 128, 96])

    def forward(self, x, edge_index, edge_attr, initial_x, att_edge_attr):
        from .mp_layer import mp_layer_forward
        return mp_layer_forward(self, "clr", x, edge_index, edge_attr, initial_x, att_edge_attr)


def modality_present(feats: torch.Tensor) -> torch.Tensor:
    """clr_att_gnn.py:107-121: node n has the modality iff the sum of its row is non-zero."""
    n = feats.size(0)
    if n == 0:
        return torch.empty(0, dtype=torch.bool, device=feats.device)
    f = feats.reshape(n, -1).contiguous()
    _lib.require_cuda(f, "modality features", torch.float32)
    has = torch.empty(n, dtype=torch.uint8, device=f.device)
    _lib.check(_lib.load().b3d_modality_mask(f.data_ptr(), n, f.size(1), has.data_ptr(), _lib.current_stream(f.device)),
               "b3d_modality_mask")
    return has.bool()


def _modality_rows_enqueue(feats: torch.Tensor):
    """The two launches of ``b3d_modality_rows`` on the current stream, nothing read back: (rows [n] int64, count [1] int32), or
    None for an empty batch."""
    n = feats.size(0)
    if n == 0:                                        # empty batch: no rows (reshape(0, -1) cannot infer the width)
        return None
    f = feats.reshape(n, -1).contiguous()
    _lib.require_cuda(f, "modality features", torch.float32)
    has = torch.empty(max(n, 1), dtype=torch.uint8, device=f.device)
    rows = torch.empty(max(n, 1), dtype=torch.int64, device=f.device)
    count = torch.empty(1, dtype=torch.int32, device=f.device)
    _lib.check(_lib.load().b3d_modality_rows(f.data_ptr(), n, f.size(1), has.data_ptr(), rows.data_ptr(), count.data_ptr(),
                                             _lib.current_stream(f.device)), "b3d_modality_rows")
    return rows, count


def modality_row_ids(feats: torch.Tensor) -> torch.Tensor:
    """``torch.nonzero(modality_present(feats)).squeeze(1)`` (int64, ascending) from two HIP launches (``b3d_modality_rows``:
    the presence mask, then a one-workgroup ballot / scan compaction).  The count is a shape: one read-back, on the
    current stream."""
    if feats.size(0) == 0:
        return torch.empty(0, dtype=torch.int64, device=feats.device)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("modality_row_ids reads the row count back to the host and cannot run inside a stream capture: "
                           "pass rows=modality_rows(data) computed in front of it")
    rows, count = _modality_rows_enqueue(feats)
    return rows[: int(count.item())]


class PendingRows:
    """Handle of ``GNN.modality_rows_begin``: the compactions are enqueued, their counts on their way to pinned host memory."""
    __slots__ = ("parts", "host", "event", "stream", "device")


def _param_list(m: "GNN") -> List[torch.Tensor]:
    out: List[torch.Tensor] = []
    for seq in (m.edge_encoder, m.node_encoder, m.edge_classifier, m.fc_lidar_encoder, m.fc_radar_encoder):
        for lin in _linears(seq):
            out += [lin.weight, lin.bias]
    for att in (m.c2c_att, m.l2l_att, m.r2r_att):
        out += [att.in_proj_weight, att.in_proj_bias, att.out_proj.weight, att.out_proj.bias]
    for seq in (m.att_edge_encoder, m.message_passing.edge_update, m.message_passing.create_past_msgs,
                m.message_passing.create_future_msgs, m.message_passing.combine_future_past):
        for lin in _linears(seq):
            out += [lin.weight, lin.bias]
    return out


def _fill(dst, tensors, k):
    for i in range(len(dst)):
        dst[i].w = tensors[k + 2 * i].data_ptr()
        dst[i].b = tensors[k + 2 * i + 1].data_ptr()
    return k + 2 * len(dst)


def _fill_mha(dst, tensors, k):
    dst.in_proj_weight, dst.in_proj_bias, dst.out_proj_weight, dst.out_proj_bias = (tensors[k + i].data_ptr() for i in range(4))
    return k + 4


def _clr_struct(cls, t):
    s = cls()
    k = 0
    k = _fill(s.edge_encoder, t, k)
    k = _fill(s.node_encoder, t, k)
    k = _fill(s.edge_classifier, t, k)
    k = _fill(s.fc_lidar_encoder, t, k)
    k = _fill(s.fc_radar_encoder, t, k)
    k = _fill_mha(s.c2c_att, t, k)
    k = _fill_mha(s.l2l_att, t, k)
    k = _fill_mha(s.r2r_att, t, k)
    k = _fill(s.att_edge_encoder, t, k)
    k = _fill(s.mp.edge_update, t, k)
    k = _fill(s.mp.create_past_msgs, t, k)
    k = _fill(s.mp.create_future_msgs, t, k)
    k = _fill(s.mp.combine_future_past, t, k)
    assert k == len(t)
    return s


_ENC_STREAMS = {}


class _GNNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, graph, pose_feats, edge_attr, node_timestamps, x_img, pointnet_out, lidar_nodes,
                radarnet_out, radar_nodes, training, ready, *params):
        lib = _lib.load()
        dev = pose_feats.device
        N, E = graph.N, graph.E
        nl, nr = int(lidar_nodes.numel()), int(radar_nodes.numel())
        single = module.single_stream or not _lib.forks_allowed()
        flags = ((B3D_FLAG_TRAINING if training else 0) | (B3D_FLAG_RUN_DEAD_KNN if module.run_dead_knn else 0)
                 | (B3D_FLAG_SINGLE_STREAM if single else 0)
                 | (0 if getattr(module, "run_dead_last_messages", True) else B3D_FLAG_SKIP_DEAD_LAST_MESSAGES))
        # optional: let the discarded k-NN block run on under the loss and the backward sweep (measured on
        # MI355X: 4 % slower than joining at the end of forward -- it delays the start of every backward kernel)
        defer = bool(training and module.run_dead_knn and not single and module.defer_knn_join)
        if defer:
            flags |= B3D_FLAG_DEFER_SIDE_JOIN
        nbytes = lib.b3d_clr_workspace_bytes(N, E, nl, nr, module.depth, flags)
        if nbytes == 0:
            raise ValueError(f"unsupported gnn_depth {module.depth} (1..15)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ctx.save_for_backward(*params)                           # version-checked: in-place edits before backward are errors
        params = [p.detach() for p in params]
        w = _clr_struct(_lib.b3d_clr_weights, params)
        kc = module.knn_conv
        gat = [kc.lin_src.weight.detach(), kc.att_src.detach().reshape(-1), kc.att_dst.detach().reshape(-1), kc.bias.detach()]
        w.knn_conv.lin, w.knn_conv.att_src, w.knn_conv.att_dst, w.knn_conv.bias = (t.data_ptr() for t in gat)
        inp = _lib.b3d_clr_inputs()
        inp.pose_feats, inp.edge_attr, inp.node_timestamps = pose_feats.data_ptr(), edge_attr.data_ptr(), node_timestamps.data_ptr()
        inp.x_img = x_img.data_ptr()
        inp.pointnet_out, inp.lidar_nodes, inp.n_lidar = (pointnet_out.data_ptr() if nl else None), (lidar_nodes.data_ptr() if nl else None), nl
        inp.radarnet_out, inp.radar_nodes, inp.n_radar = (radarnet_out.data_ptr() if nr else None), (radar_nodes.data_ptr() if nr else None), nr
        # event behind the frozen encoders (GNN._encode): the forward waits for it right before it reads their outputs
        inp.encoders_ready = ready.cuda_event if ready is not None else None
        prob = torch.empty((E, 1), dtype=torch.float32, device=dev)
        x_sens = torch.empty((N, 288), dtype=torch.float32, device=dev)
        _lib.check(lib.b3d_clr_forward(C.byref(w), C.byref(graph.c), C.byref(inp), module.depth, flags, ws.data_ptr(), nbytes,
                                       prob.data_ptr(), x_sens.data_ptr(), _lib.current_stream(dev)), "b3d_clr_forward")
        ctx.set_materialize_grads(False)
        ctx.module, ctx.graph, ctx.ws, ctx.nbytes, ctx.flags = module, graph, ws, nbytes, flags
        ctx.ws_owner = _lib.Workspace(ws, defer)
        ctx.inp, ctx.keep = inp, (gat, pose_feats, edge_attr, node_timestamps, x_img, pointnet_out,
                                                      lidar_nodes, radarnet_out, radar_nodes, ready)
        module._last_workspace = (ws, nbytes, flags, N, E, nl, nr) if module.keep_workspace else None
        return prob, x_sens

    @staticmethod
    def backward(ctx, d_prob, d_x_sens):
        lib = _lib.load()
        if not (ctx.flags & B3D_FLAG_TRAINING):
            raise RuntimeError("backward through a GNN forward that ran without gradient tracking")
        params = [p.detach() for p in ctx.saved_tensors]
        dev = params[0].device
        if d_prob is not None:
            d_prob = d_prob.contiguous().float()
        if d_x_sens is not None:
            d_x_sens = d_x_sens.contiguous().float()
        sink = getattr(ctx.module, "_grad_sink", None)      # optim.FlatAdam: gradients land in its flat buffer
        grads = sink.targets() if sink is not None else [torch.empty_like(p) for p in params]
        w = _clr_struct(_lib.b3d_clr_weights, params)
        g = _clr_struct(_lib.b3d_clr_grads, grads)
        _lib.check(lib.b3d_clr_backward(C.byref(w), C.byref(ctx.graph.c), C.byref(ctx.inp), ctx.module.depth, ctx.ws.data_ptr(),
                                        ctx.nbytes, _lib.ptr(d_prob), _lib.ptr(d_x_sens), C.byref(g), _lib.current_stream(dev)),
                   "b3d_clr_backward")
        ctx.ws_owner.joined()              # backward joined the library's side stream into this stream
        if sink is not None:
            sink.deposited()
            return (None,) * (12 + len(params))
        return (None,) * 12 + tuple(grads)


def _first_k(mask: torch.Tensor, k: int) -> torch.Tensor:
    """Ascending positions of the first ``k`` True entries of ``mask`` -- ``torch.nonzero(mask)[:k]`` without its read-back of
    the result's size (``k`` is known to the caller)."""
    return torch.argsort(~mask, stable=True)[:k]


class EmbeddingCache:
    """Encoder outputs of the detections of a scene, keyed by global node id: every detection is
    encoded ONCE per scene instead of once per window it appears in -- with the reference's stride-1 windows of
    ``batch_size_graph`` frames (predict.py:172) up to 5x fewer encoder rows.  ``clear()`` between scenes (ids are per scene,
    predict.py:595-611).

    Round 4: everything lives on the device.  ``ids`` is a SORTED int64 table, a lookup is ``torch.searchsorted``; the encoder
    outputs are dense tables in id order (rows without the modality are zero) beside two presence masks.  No Python
    dictionary, no per-detection loop; the host reads back sizes only -- one synchronisation per ``add`` (how many ids are
    new and how many of those carry LiDAR / radar points: the encoder batches' shapes), one per ``window`` (how many of its
    rows carry them: the shapes ``b3d_clr_forward`` takes), or, through ``add_windows`` / ``windows``, three per SCENE."""

    def __init__(self, capacity: int = 0):
        self.capacity = capacity            # kept for the round-3 signature; tables are sized by their content
        self.clear()

    def clear(self):
        self.ids = None                     # [U] int64, ascending
        self.img = self.lidar = self.radar = self.has_lidar = self.has_radar = None
        self.hits = self.misses = 0
        self.encoder_rows = {"img": 0, "lidar": 0, "radar": 0}

    def __len__(self):
        return 0 if self.ids is None else int(self.ids.numel())

    # ---- lookups --------------------------------------------------------------------------------------------------------
    def rows_of(self, node_ids: torch.Tensor):
        """(row of every id in the tables, hit mask); a miss has an arbitrary valid row."""
        if self.ids is None or self.ids.numel() == 0:
            return torch.zeros_like(node_ids), torch.zeros_like(node_ids, dtype=torch.bool)
        pos = torch.searchsorted(self.ids, node_ids).clamp_(max=self.ids.numel() - 1)
        return pos, self.ids[pos] == node_ids

    # ---- filling ----------------------------------------------------------------------------------------------------------
    def add(self, model: "GNN", node_ids: torch.Tensor, img_feats, lidar_feats, radar_feats, chunk: int = 8192):
        """Encode the detections of ``node_ids`` (int64, on the device; duplicates allowed) that the tables do not hold yet."""
        if model.resnet.training or model.pointnet.training or model.radarnet.training:
            raise RuntimeError("the embedding cache needs the encoders in eval mode: in train mode their BatchNorm "
                               "statistics depend on which rows share a batch")
        dev = node_ids.device
        m = node_ids.numel()
        if m == 0:
            return
        # first occurrence of every distinct id of the request, in id order; drop those the tables hold
        uniq, inv = torch.unique(node_ids, return_inverse=True)
        first = torch.full((uniq.numel(),), m, dtype=torch.long, device=dev).scatter_reduce_(0, inv, torch.arange(m, device=dev), "amin")
        _, hit = self.rows_of(uniq)
        new = ~hit
        lid_rows = lidar_feats.reshape(m, -1)
        rad_rows = radar_feats.reshape(m, -1)
        has_l = modality_present(lidar_feats)[first] & new
        has_r = modality_present(radar_feats)[first] & new
        n_new, n_l, n_r = (int(v) for v in torch.stack([new.sum(), has_l.sum(), has_r.sum()]).tolist())      # the one read-back
        self.hits += m - n_new
        self.misses += n_new
        if n_new == 0:
            return
        sel = _first_k(new, n_new)                                   # positions in `uniq` of the new ids, ascending = id order
        src = first[sel]                                             # their rows in the request
        img = torch.empty((n_new, 96), dtype=torch.float32, device=dev)
        lidar = torch.zeros((n_new, 256), dtype=torch.float32, device=dev)
        radar = torch.zeros((n_new, 256), dtype=torch.float32, device=dev)
        hl, hr = has_l[sel], has_r[sel]
        li, ri = _first_k(hl, n_l), _first_k(hr, n_r)                 # rows of the NEW block that carry the modality
        with torch.no_grad():
            for c0 in range(0, n_new, chunk):
                img[c0:c0 + chunk] = model.resnet.encode(img_feats[src[c0:c0 + chunk]]).float()
            for c0 in range(0, n_l, chunk):
                rr = li[c0:c0 + chunk]
                lidar[rr] = model.pointnet.forward_feat(lid_rows[src[rr]].view(-1, 3, 128)).float()
            for c0 in range(0, n_r, chunk):
                rr = ri[c0:c0 + chunk]
                radar[rr] = model.radarnet.forward_feat(rad_rows[src[rr]].view(-1, 4, 64)).float()
        self.encoder_rows["img"] += n_new
        self.encoder_rows["lidar"] += n_l
        self.encoder_rows["radar"] += n_r
        new_ids = uniq[sel]
        if self.ids is None or self.ids.numel() == 0:
            self.ids, self.img, self.lidar, self.radar, self.has_lidar, self.has_radar = new_ids, img, lidar, radar, hl, hr
            return
        # merge two sorted id lists: one stable sort of the concatenation (old ids first), tables permuted alike
        ids = torch.cat([self.ids, new_ids])
        order = torch.argsort(ids, stable=True)
        self.ids = ids[order]
        self.img = torch.cat([self.img, img])[order]
        self.lidar = torch.cat([self.lidar, lidar])[order]
        self.radar = torch.cat([self.radar, radar])[order]
        self.has_lidar = torch.cat([self.has_lidar, hl])[order]
        self.has_radar = torch.cat([self.has_radar, hr])[order]

    def add_windows(self, model: "GNN", windows, ids_of=None):
        """All windows of a scene in one ``add``: only the rows a window contributes for the FIRST time are gathered, so the
        request is the scene's detections once, not five times (two read-backs for the whole scene)."""
        ids_of = ids_of or window_node_ids
        dev = windows[0].pose_feats.device
        gids = [ids_of(w).to(dev) for w in windows]
        sizes = [int(g.numel()) for g in gids]
        allg = torch.cat(gids)
        m = allg.numel()
        uniq, inv = torch.unique(allg, return_inverse=True)
        first = torch.full((uniq.numel(),), m, dtype=torch.long, device=dev).scatter_reduce_(0, inv, torch.arange(m, device=dev), "amin")
        pos = torch.sort(first).values                               # first occurrences in concatenation (= window) order
        off = [0]
        for n_ in sizes:
            off.append(off[-1] + n_)
        bounds = torch.searchsorted(pos, torch.tensor(off, device=dev)).tolist()          # read-back 1 of the scene
        idx = [pos[bounds[k]:bounds[k + 1]] - off[k] for k in range(len(windows))]       # rows of window k nobody held before
        live = [k for k in range(len(windows)) if bounds[k + 1] > bounds[k]]
        pick = lambda name: torch.cat([getattr(windows[k], name)[idx[k]] for k in live])          # noqa: E731
        self.add(model, allg[pos], pick("img_feats"), pick("lidar_feats"), pick("radar_feats"))

    # ---- reading --------------------------------------------------------------------------------------------------------
    def window(self, node_ids: torch.Tensor, counts=None):
        """The ``encoded`` tuple of ``GNN.forward`` for the detections ``node_ids`` (all must be cached).  ``counts``: (rows with
        LiDAR, rows with radar) if the caller already holds them (``windows``); otherwise one read-back."""
        rows, hit = self.rows_of(node_ids)
        hl, hr = self.has_lidar[rows], self.has_radar[rows]
        if counts is None:
            n_l, n_r, n_hit = (int(v) for v in torch.stack([hl.sum(), hr.sum(), hit.sum()]).tolist())
            if n_hit != node_ids.numel():
                raise KeyError(f"{node_ids.numel() - n_hit} detections of this window are not in the embedding cache")
        else:
            n_l, n_r = counts
        ln, rn = _first_k(hl, n_l), _first_k(hr, n_r)
        return (self.img[rows].contiguous(), self.lidar[rows[ln]].contiguous(), ln.to(torch.int32).contiguous(),
                self.radar[rows[rn]].contiguous(), rn.to(torch.int32).contiguous())

    def scene_tables(self, list_of_node_ids):
        """The encoder outputs of ALL windows of a scene back to back, with ONE read-back (the LiDAR / radar row counts of every
        window together): a dict with ``img`` [M, 96] (window after window), ``lidar`` [NL, 256] / ``radar`` [NR, 256] (the rows
        that carry the modality, same order), ``lidar_nodes`` / ``radar_nodes`` (their node index INSIDE their window, int32),
        ``off`` / ``loff`` / ``roff`` (host lists: where window k starts in each).  A run of consecutive windows is a slice."""
        dev = self.ids.device
        sizes = [int(i.numel()) for i in list_of_node_ids]
        if not sizes or min(sizes) == 0:
            raise ValueError("scene_tables: every window needs at least one detection")
        off = [0]
        for n_ in sizes:
            off.append(off[-1] + n_)
        allg = torch.cat([i.to(dev) for i in list_of_node_ids])
        m = allg.numel()
        rows, hit = self.rows_of(allg)
        hl, hr = self.has_lidar[rows], self.has_radar[rows]
        offt = torch.tensor(off, device=dev)
        cl, cr = torch.cumsum(hl, 0), torch.cumsum(hr, 0)
        zero = torch.zeros(1, dtype=cl.dtype, device=dev)
        ends = offt[1:] - 1
        vals = torch.cat([torch.cat([zero, cl[ends]]), torch.cat([zero, cr[ends]]), (~hit).sum().reshape(1)]).tolist()     # the read-back
        w = len(sizes)
        loff, roff, miss = [int(v) for v in vals[:w + 1]], [int(v) for v in vals[w + 1:2 * w + 2]], int(vals[-1])
        if miss:
            raise KeyError(f"{miss} detections of these windows are not in the embedding cache")
        win_start = torch.repeat_interleave(offt[:-1], torch.tensor(sizes, device=dev), output_size=m)
        pl, pr = _first_k(hl, loff[-1]), _first_k(hr, roff[-1])       # positions (concatenation order) of the rows with the modality
        return {"img": self.img[rows], "lidar": self.lidar[rows[pl]], "radar": self.radar[rows[pr]],
                "lidar_nodes": (pl - win_start[pl]).to(torch.int32), "radar_nodes": (pr - win_start[pr]).to(torch.int32),
                "off": off, "loff": loff, "roff": roff}

    @staticmethod
    def tables_slice(t, k0: int, k1: int):
        """The ``encoded`` tuple of ``GNN.forward`` for windows k0 .. k1-1 of ``scene_tables`` scored as ONE disjoint-union graph."""
        o, lo, ro = t["off"], t["loff"], t["roff"]
        ln, rn = t["lidar_nodes"][lo[k0]:lo[k1]], t["radar_nodes"][ro[k0]:ro[k1]]
        if k1 - k0 > 1:                                              # node indices of the union graph: + the window's offset in it
            dev = ln.device
            starts = torch.tensor([o[k] - o[k0] for k in range(k0, k1)], dtype=torch.int32, device=dev)
            ln = ln + torch.repeat_interleave(starts, torch.tensor([lo[k + 1] - lo[k] for k in range(k0, k1)], device=dev), output_size=lo[k1] - lo[k0])
            rn = rn + torch.repeat_interleave(starts, torch.tensor([ro[k + 1] - ro[k] for k in range(k0, k1)], device=dev), output_size=ro[k1] - ro[k0])
        return (t["img"][o[k0]:o[k1]], t["lidar"][lo[k0]:lo[k1]], ln.contiguous(), t["radar"][ro[k0]:ro[k1]], rn.contiguous())

    def windows(self, list_of_node_ids):
        """``window`` for every window of a scene with ONE read-back (``scene_tables``)."""
        t = self.scene_tables(list_of_node_ids)
        return [self.tables_slice(t, k, k + 1) for k in range(len(list_of_node_ids))]


def window_node_ids(data) -> torch.Tensor:
    """Global (scene-level) ids of a window's detections: ``data.global_ids`` if present, else the first column of
    ``data.global_node_timestamps`` (utils/graph_data.py:190)."""
    g = getattr(data, "global_ids", None)
    if g is None:
        g = data.global_node_timestamps[:, 0]
    return g.to(torch.int64)


class GNN(nn.Module):
    """``GNN(img_encoder, lidar_encoder, radar_encoder, use_attention=True, gnn_depth=6, edge_dim=64,
    node_dim=179)`` -- reference clr_att_gnn.py:16-188.

    ``forward(data)`` reads ``pose_feats [N,19]``, ``img_feats [N,3,32,32]``, ``lidar_feats [N,128,3]``,
    ``radar_feats [N,64,4]``, ``edge_index [2,E] i64``, ``edge_attr [E,4]``, ``node_timestamps [N]`` and
    returns ``(edge_prob [E,1] after the sigmoid, x_sens [N,288] = x_img | x_lidar | x_radar)``.
    The reference's ``use_attention=False`` branch is a shape error as shipped (clr_att_gnn.py:166-170
    feeds 512 features into ``Linear(640, ...)``) and raises ``NotImplementedError`` here.
    """

    def __init__(self, img_encoder, lidar_encoder, radar_encoder, use_attention=True, gnn_depth=6, edge_dim=64,
                 node_dim=179):
        super().__init__()
        self.depth = gnn_depth
        self.use_attention = use_attention
        self.resnet, self.pointnet, self.radarnet = img_encoder, lidar_encoder, radar_encoder
        for enc in (self.resnet, self.pointnet, self.radarnet):          # clr_att_gnn.py:26-33
            for p in enc.parameters():
                p.requires_grad = False
        self.edge_encoder = _mlp([4, 16, 32, 64], inplace_relu=True)
        self.node_encoder = _mlp([19, 48, 96])
        cls = list(_mlp([64, 32, 16, 8, 1])) + [nn.Sigmoid()]
        self.edge_classifier = nn.Sequential(*cls)
        self.fc_lidar_encoder = _mlp([256, 192, 128], inplace_relu=True)
        self.fc_radar_encoder = _mlp([256, 192, 128, 64], inplace_relu=True)
        self.message_passing = CausalMessagePassing()
        self.c2c_att = nn.MultiheadAttention(embed_dim=96, num_heads=2, kdim=96, vdim=96, batch_first=True)
        self.l2l_att = nn.MultiheadAttention(embed_dim=128, num_heads=2, kdim=128, vdim=128, batch_first=True)
        self.r2r_att = nn.MultiheadAttention(embed_dim=64, num_heads=2, kdim=64, vdim=64, batch_first=True)
        self.att_edge_encoder = _mlp([640, 512, 384, 256, 128, 64])
        self.knn_conv = GATConvParams(96)
        self.run_dead_knn = True
        # True (default): every kernel on the caller's stream.  False: the discarded k-NN block runs on the
        # library's side stream (worth ~4 % before the first layers were hoisted; now it only adds jitter)
        self.single_stream = True
        self.defer_knn_join = False    # True: B3D_FLAG_DEFER_SIDE_JOIN in training forwards
        # The last layer's create_future_msgs / create_past_msgs / combine_future_past feed nothing (clr_att_gnn.py:188 returns
        # edge_classifier(edge_attr)); the reference executes them, and so does this model by default.  False skips them
        # (B3D_FLAG_SKIP_DEAD_LAST_MESSAGES): outputs and gradients are bit-identical.
        self.run_dead_last_messages = True
        self.keep_workspace = False
        self._last_workspace = None
        self.mask_stream = None         # see modality_rows()
        # True (default): the three frozen encoders of a forward run side by side -- ResNetAE (vector-ALU convolutions), then
        # RadarNet, on a side stream under PointNet (MFMA-bound point stacks) on the caller's stream, joined before the
        # first kernel that reads their outputs.  Same kernels, same bits; see encode_modalities().
        self.encoder_streams = True
        self._grad_sink = None          # set by optim.FlatAdam: backward writes gradients into its flat buffer
        # Non-reference: True USES the k-NN + GAT block's result (layers 0, 2, 4; clr_att_gnn.py:178-184 computes and drops it)
        # and trains ``knn_conv``: see _forward_writeback
        self.knn_writeback = False
        self._last_knn = None

    def _forward_writeback(self, data, encoded=None, rows=None):
        """``knn_writeback=True``: the layer loop in Python over the library's operators -- frozen encoders (HIP), the k-NN + GAT
        block with its backward (``_lib.knn_gat_conv``), the CausalMessagePassing layer operator (``mp_layer``), the dense
        stacks (modality heads, att_edge_encoder, edge / node encoder, classifier) through ``_lib.mlp`` (b3d_mlp_forward /
        _backward) and the one-key attention's per-node ``out_proj(v_proj(.))`` through ``_lib.xattn_node_affine``
        (b3d_xattn_node_affine_*): no ``nn.Linear`` / ``nn.MultiheadAttention`` forward runs.  PyTorch keeps the index plumbing
        (row scatters of the modality heads, the per-edge gather + concatenation in front of att_edge_encoder).  The whole-model
        entry point cannot be used: the per-node tables of its hoisted first layers are produced from the x the block would
        replace."""
        pose_feats, edge_index, node_timestamps = data.pose_feats, data.edge_index, data.node_timestamps
        _lib.require_cuda(pose_feats, "data.pose_feats", torch.float32)
        if edge_index.size(1) == 0 or pose_feats.size(0) == 0:
            raise ValueError("empty graph: the reference's callers skip these (predict.py:179-180)")
        n = pose_feats.size(0)
        if encoded is None:
            encoded = self._encode(data, rows, join=True)[0]
        x_img, pointnet_out, lidar_nodes, radarnet_out, radar_nodes = encoded
        e = _lib.mlp(self.edge_encoder, data.edge_attr.float().contiguous())
        x_lidar = x_img.new_zeros((n, 128))
        x_radar = x_img.new_zeros((n, 64))
        if lidar_nodes.numel():
            x_lidar = x_lidar.index_copy(0, lidar_nodes.long(), _lib.mlp(self.fc_lidar_encoder, pointnet_out.contiguous()))
        if radar_nodes.numel():
            x_radar = x_radar.index_copy(0, radar_nodes.long(), _lib.mlp(self.fc_radar_encoder, radarnet_out.contiguous()))
        # MultiheadAttention with ONE key: softmax == 1, the output is out_proj(v_proj(value)) of the value's node
        s = torch.cat([_lib.xattn_node_affine(self.r2r_att, x_radar), _lib.xattn_node_affine(self.l2l_att, x_lidar),
                       _lib.xattn_node_affine(self.c2c_att, x_img.contiguous())], 1)
        att = _lib.mlp(self.att_edge_encoder, torch.cat([s[edge_index[1]], s[edge_index[0]], e], 1))     # x_sens_i | x_sens_j | edge_attr
        x_sens = torch.cat([x_img, x_lidar, x_radar], 1)
        x0 = _lib.mlp(self.node_encoder, pose_feats)
        x = x0
        self._last_knn = []
        for i in range(self.depth):
            if i % 2 == 0:
                x, nbr, cnt = _lib.knn_gat_conv(x.contiguous(), node_timestamps, self.knn_conv, 20, return_graph=True)
                self._last_knn.append((nbr, cnt))
            x, e = self.message_passing(x.contiguous(), edge_index, e.contiguous(), x0.contiguous(), att.contiguous())
        return _lib.mlp(self.edge_classifier, e.contiguous()), x_sens

    def _hip_params(self):
        """Parameters whose gradients ``backward`` of the HIP path produces, in C-ABI struct order."""
        return _param_list(self)

    def modality_rows(self, data):
        """clr_att_gnn.py:107-121 as two launches (``b3d_modality_mask``) and two compactions: the node ids
        (int64, ascending) of the rows that carry LiDAR / radar points.  The row COUNTS are shapes downstream
        (the encoders run on the compacted rows, :131,139), so they must reach the host: one synchronisation.

        With ``self.mask_stream`` set (a ``torch.cuda.Stream``) the masks run there and only that stream is
        waited for, so the caller's stream keeps its queue -- the host can enqueue step k+1 while step k runs.
        A batch from ``graph_data``'s prefetching loader carries the event of its H2D copy (``_b3d_ready_event``) and the
        side stream waits for it; for any other producer the caller guarantees that ``lidar_feats`` / ``radar_feats`` are
        complete when this is called (resident inputs).

        ``modality_rows_begin`` / ``modality_rows_end`` are the two halves: a loop that begins batch k + 1 BEFORE it launches
        step k never waits for the counts (HIP multiplexes its streams onto four hardware queues: enqueued behind a running
        step the side stream's launches wait for that step, and so does the host -- 50 us of idle GPU per step, round 5)."""
        lidar_feats, radar_feats = data.lidar_feats, data.radar_feats
        if self.mask_stream is None or torch.cuda.is_current_stream_capturing() or not lidar_feats.is_cuda:
            return modality_row_ids(lidar_feats), modality_row_ids(radar_feats)
        return self.modality_rows_end(self.modality_rows_begin(data))

    def modality_rows_into(self, data, static_rows, mismatch: torch.Tensor) -> None:
        """``modality_rows`` without a host read-back, for a caller that has fixed the two counts beforehand -- a hipGraph-captured
        step, where they are the shapes of everything behind them: the row ids of ``data`` are written into ``static_rows`` =
        (lidar ids [nl], radar ids [nr]) (int64, device) on the CURRENT stream (capturable), and ``mismatch`` (int32 [1], device) is
        incremented for each modality whose real count differs from the buffer's length.  The caller reads ``mismatch`` whenever it
        next synchronises (``bench.py``: after the timed region) -- the replay of a graph on a batch with other counts must fail
        loudly, just not per step.  Replaces the prologue's ``.item()`` (clr_att_gnn.py:107-121 is ``torch.nonzero``, a read-back)."""
        lib = _lib.load()
        if mismatch.dtype != torch.int32 or mismatch.numel() != 1 or not mismatch.is_cuda:
            raise ValueError("modality_rows_into: mismatch must be a CUDA int32 tensor with one element")
        for feats, dst in ((data.lidar_feats, static_rows[0]), (data.radar_feats, static_rows[1])):
            n = feats.size(0)
            if dst.dtype != torch.int64 or not dst.is_cuda or not dst.is_contiguous() or dst.numel() > n:
                raise ValueError("modality_rows_into: static row buffers must be contiguous CUDA int64 tensors of at most N entries")
            if n == 0:
                continue
            f = feats.reshape(n, -1).contiguous()
            _lib.require_cuda(f, "modality features", torch.float32)
            has = torch.empty(n, dtype=torch.uint8, device=f.device)
            count = torch.empty(1, dtype=torch.int32, device=f.device)
            # (a zero-length buffer still gets a valid pointer: the kernel writes nothing past `expected`)
            rows_ptr = dst.data_ptr() if dst.numel() else has.data_ptr()
            _lib.check(lib.b3d_modality_rows_expect(f.data_ptr(), n, f.size(1), has.data_ptr(), rows_ptr, int(dst.numel()),
                                                    count.data_ptr(), mismatch.data_ptr(), _lib.current_stream(f.device)),
                       "b3d_modality_rows_expect")

    def modality_rows_begin(self, data) -> PendingRows:
        """Enqueue the masks + compactions of ``data`` (on ``self.mask_stream`` if set) and the copy of the two counts to pinned
        host memory; nothing waits.  ``modality_rows_end`` returns the row ids."""
        lidar_feats, radar_feats = data.lidar_feats, data.radar_feats
        dev = lidar_feats.device
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("modality_rows_begin reads row counts back to the host and cannot run inside a stream capture")
        cur = torch.cuda.current_stream(dev)
        ms = self.mask_stream if self.mask_stream is not None else cur
        ev = getattr(data, "_b3d_ready_event", None)      # set by graph_data's prefetching loader: the H2D copy of this batch
        if ev is not None:
            ms.wait_event(ev)
        h = PendingRows()
        h.stream, h.device = ms, dev
        h.host = torch.zeros(2, dtype=torch.int32).pin_memory()
        with torch.cuda.stream(ms):
            h.parts = (_modality_rows_enqueue(lidar_feats), _modality_rows_enqueue(radar_feats))
            for j, part in enumerate(h.parts):
                if part is not None:
                    h.host[j:j + 1].copy_(part[1], non_blocking=True)
            h.event = torch.cuda.Event()
            h.event.record(ms)
        return h

    def modality_rows_end(self, h: PendingRows):
        """The row ids of a ``modality_rows_begin``: waits for ITS event only, then orders the caller's stream behind it."""
        h.event.synchronize()
        cur = torch.cuda.current_stream(h.device)
        cur.wait_event(h.event)
        out = []
        for j, part in enumerate(h.parts):
            if part is None:
                out.append(torch.empty(0, dtype=torch.int64, device=h.device))
                continue
            t = part[0][: int(h.host[j])]
            if h.stream is not cur:
                t.record_stream(cur)
            out.append(t)
        return out[0], out[1]

    def encode_modalities(self, data, cache: "Optional[EmbeddingCache]" = None, node_ids=None, rows=None):
        """The frozen, adjacent part (clr_att_gnn.py:107-141): presence masks, ResNet / PointNet /
        RadarNet embeddings of the rows that have the modality, and the sticky ``.eval()`` switch
        when fewer than two rows have it.  ``rows``: the result of ``modality_rows(data)`` if the caller
        already holds it.

        With ``cache`` (inference: every encoder in eval mode) a detection is encoded once per scene instead of
        once per window it appears in -- with the reference's stride-1 windows of ``batch_size_graph`` frames
        (predict.py:172) that is up to 5x fewer encoder rows.  ``node_ids`` are the detections' global ids
        (default: ``data.global_node_timestamps[:, 0]``, graph_data.py:190)."""
        if cache is not None:
            return self._encode_cached(data, cache, node_ids)
        return self._encode(data, rows, join=True)[0]

    def _encode(self, data, rows, join: bool):
        """(outputs of encode_modalities, event or None).  ``join=False`` (used by ``forward``): nothing is joined back into
        the caller's stream -- PointNet, too, runs on a side stream, and the returned event (recorded behind all three
        encoders) is handed to ``b3d_clr_forward`` (``b3d_clr_inputs.encoders_ready``), which waits for it only after the
        part of the forward that does not read encoder outputs: weight images, edge / node encoder, layer 0's per-node table
        and the first k-NN block run on the caller's stream WHILE the encoders run."""
        img_feats, lidar_feats, radar_feats = data.img_feats, data.lidar_feats, data.radar_feats
        lidar_nodes, radar_nodes = rows if rows is not None else self.modality_rows(data)
        # The encoders do not depend on each other: with `encoder_streams` the camera and radar encoders are enqueued on a
        # side stream (forked from, and joined back into, the caller's stream: inside a stream capture a parallel branch of
        # the graph) next to PointNet -- the longest of the three.  One side stream for ResNetAE and RadarNet: with a stream
        # of its own RadarNet's branch started late in the replay (behind PointNet's kernels) and ended on the critical
        # path; behind ResNetAE it is done well before PointNet (4.87 -> 4.75 ms per step).  The Python call order -- and
        # with it the order in which the Dropout layers draw from the generator -- is the sequential one.  No
        # record_stream: every use of a side stream starts by waiting for the caller's stream, so a block of its pool is
        # never reused while an earlier consumer reads it.
        dev = img_feats.device
        side = pn = None
        if self.encoder_streams and img_feats.is_cuda and _lib.forks_allowed():
            streams = _ENC_STREAMS.get(dev)          # per device, shared by all models of the process (a module attribute would
            if streams is None:                      # make the module impossible to deepcopy / pickle once it has run)
                streams = _ENC_STREAMS[dev] = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
            cur = torch.cuda.current_stream(dev)
            side = streams[0]
            side.wait_stream(cur)
            if not join:
                pn = streams[1]
                pn.wait_stream(cur)
        import contextlib
        on = lambda st: torch.cuda.stream(st) if st is not None else contextlib.nullcontext()
        with torch.no_grad():
            with on(side):
                x_img = self.resnet.encode(img_feats).float().contiguous()
            if lidar_nodes.numel() < 2:
                self.pointnet.eval()
                self.fc_lidar_encoder.eval()
            with on(pn):
                pointnet_out = self.pointnet.forward_feat(lidar_feats[lidar_nodes].view(-1, 3, 128)).float().contiguous()
            if radar_nodes.numel() < 2:
                self.radarnet.eval()
                self.fc_radar_encoder.eval()
            with on(side):
                radarnet_out = self.radarnet.forward_feat(radar_feats[radar_nodes].view(-1, 4, 64)).float().contiguous()
            lidar_i32, radar_i32 = lidar_nodes.to(torch.int32).contiguous(), radar_nodes.to(torch.int32).contiguous()
        ready = None
        if pn is not None:
            # The row ids were produced on another stream (modality_rows: the mask stream) and are read by gathers on the
            # side streams; nothing joins those into the caller's stream before this function returns and drops its
            # references, so the allocator must be told (without this the NEXT step's compaction, which waits for nobody,
            # reused the block while this step's RadarNet gather had not run yet: run-to-run differences in its statistics).
            if not torch.cuda.is_current_stream_capturing():
                lidar_nodes.record_stream(pn)
                radar_nodes.record_stream(side)
            pn.wait_stream(side)                     # one event behind all three
            ready = torch.cuda.Event()
            ready.record(pn)
        elif side is not None:
            cur.wait_stream(side)
        return (x_img, pointnet_out, lidar_i32, radarnet_out, radar_i32), ready

    def _encode_img(self, data, out=None):
        """The camera part of ``_encode`` alone (current stream).  ``out``: a static [N, 96] buffer to write into (HIP encoders)."""
        with torch.no_grad():
            if out is not None and data.img_feats.is_cuda and data.img_feats.size(0) > 0 and getattr(self.resnet, "use_hip", True) \
                    and getattr(self.resnet, "supports_out", False):
                return self.resnet.encode(data.img_feats, out=out)
            return self.resnet.encode(data.img_feats).float().contiguous()

    @staticmethod
    def _feat(enc, x, out):
        """``enc.forward_feat(x)``, written into ``out`` where the encoder can (the HIP heads of ``batch3dmot_amd.encoders``)."""
        if out is not None and x.is_cuda and x.size(0) > 0 and getattr(enc, "use_hip", True) and getattr(enc, "supports_out", False) \
                and tuple(out.shape) == (x.size(0), 256):
            return enc.forward_feat(x, out=out)
        return enc.forward_feat(x).float().contiguous()

    def _encode_lidar(self, data, lidar_nodes, out=None):
        """The LiDAR part of ``_encode`` alone (current stream): the sticky ``.eval()`` switch of an encoder that sees fewer than two
        rows (clr_att_gnn.py:128-130), PointNet, the int32 row ids."""
        with torch.no_grad():
            if lidar_nodes.numel() < 2:
                self.pointnet.eval()
                self.fc_lidar_encoder.eval()
            out = self._feat(self.pointnet, data.lidar_feats[lidar_nodes].view(-1, 3, 128), out)
            return out, lidar_nodes.to(torch.int32).contiguous()

    def _encode_radar(self, data, radar_nodes, out=None):
        """The radar part of ``_encode`` alone (clr_att_gnn.py:136-139)."""
        with torch.no_grad():
            if radar_nodes.numel() < 2:
                self.radarnet.eval()
                self.fc_radar_encoder.eval()
            out = self._feat(self.radarnet, data.radar_feats[radar_nodes].view(-1, 4, 64), out)
            return out, radar_nodes.to(torch.int32).contiguous()

    def _encode_points(self, data, rows):
        """LiDAR then radar (the reference's call order: pointnet.py's Dropout draws before radarnet.py's)."""
        lidar_nodes, radar_nodes = rows if rows is not None else self.modality_rows(data)
        return self._encode_lidar(data, lidar_nodes) + self._encode_radar(data, radar_nodes)

    def _encode_cached(self, data, cache: "EmbeddingCache", node_ids):
        if node_ids is None:
            node_ids = window_node_ids(data)
        node_ids = node_ids.to(device=data.pose_feats.device, dtype=torch.int64)
        cache.add(self, node_ids, data.img_feats, data.lidar_feats, data.radar_feats)
        return cache.window(node_ids)

    def forward(self, data, encoded=None, rows=None):
        """``encoded``: the result of ``encode_modalities(data)`` (precomputed encoder outputs); ``rows``: the result
        of ``modality_rows(data)``.  Both optional; the reference signature is ``forward(data)``."""
        if not self.use_attention:
            raise NotImplementedError("use_attention=False is a shape error in the reference "
                                      "(clr_att_gnn.py:166-170 vs :82)")
        if self.knn_writeback:
            return self._forward_writeback(data, encoded=encoded, rows=rows)
        pose_feats, edge_index, edge_attr, node_timestamps = (data.pose_feats, data.edge_index, data.edge_attr,
                                                              data.node_timestamps)
        _lib.require_cuda(pose_feats, "data.pose_feats", torch.float32)
        if pose_feats.dim() != 2 or pose_feats.size(1) != 19:
            raise ValueError(f"data.pose_feats must be [N, 19], got {tuple(pose_feats.shape)}")
        if edge_attr.dim() != 2 or edge_attr.size(1) != 4 or edge_attr.size(0) != edge_index.size(1):
            raise ValueError(f"data.edge_attr must be [E, 4], got {tuple(edge_attr.shape)}")
        if edge_index.size(1) == 0 or pose_feats.size(0) == 0:
            raise ValueError("empty graph: the reference's callers skip these (predict.py:179-180)")
        edge_attr = edge_attr.to(torch.float64).contiguous()
        node_timestamps = node_timestamps.to(torch.int64).contiguous()
        ready = None
        if encoded is None:
            # Forward-only calls (no_grad: predict.py:172-196) hand the join to b3d_clr_forward, which runs the part that
            # does not read encoder outputs underneath the encoders (+3.5 % windows per second at 2,000 / 20,000); in a
            # training step the same overlap measured 1.6 % SLOWER in round 3 and 1.0 % slower in round 4 (the train-mode statistics kernels of the point stacks
            # and the forward prefix get in each other's way), so there the encoders are joined first.
            encoded, ready = self._encode(data, rows, join=torch.is_grad_enabled())
        try:
            return self._forward_encoded(data, encoded, ready, pose_feats, edge_index, edge_attr, node_timestamps)
        except BaseException:
            # the encoders may still be running on the side streams (join=False): nothing below joined them, and the caller
            # is about to drop the tensors they read -- order the caller's stream behind them before the error travels up
            if ready is not None:
                torch.cuda.current_stream(pose_feats.device).wait_event(ready)
            raise

    def _forward_encoded(self, data, encoded, ready, pose_feats, edge_index, edge_attr, node_timestamps):
        x_img, pointnet_out, lidar_nodes, radarnet_out, radar_nodes = encoded
        graph = getattr(data, "_b3d_graph", None)
        if graph is None or graph.N != pose_feats.size(0) or graph.E != edge_index.size(1) \
                or graph._keep.data_ptr() != edge_index.data_ptr():
            graph = _lib.Graph(edge_index.contiguous(), pose_feats.size(0), validated=getattr(data, "_b3d_valid_edge_index", None) is edge_index)
            try:
                data._b3d_graph = graph
            except Exception:
                pass
        params = _param_list(self)
        for p in params:
            _lib.require_cuda(p, "parameter", torch.float32)
        training = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return _GNNFunction.apply(self, graph, pose_feats, edge_attr, node_timestamps, x_img, pointnet_out, lidar_nodes,
                                  radarnet_out, radar_nodes, training, ready, *params)
