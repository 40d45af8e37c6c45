"""On-device graph rollout buffer — stands in for the reference's
``gsmarl/utils/graph_separated_buffer.py`` (SOURCES.txt:33; SURVEY.md §8(f)
next #2) on the storage side.

The reference copies every step's observations (node features, dense
adjacency, agent ids, rewards, costs, masks) from the env processes into host
NumPy arrays. Here the episode lives in HBM and the env writes each step's
outputs *directly* into the step's slot (``gsm_step_into``: the kernels'
output pointers are redirected, so there is no copy at all), either eagerly
between policy calls or for a whole pre-generated action sequence as one HIP
graph (``gsm_graph_capture_into``).

Storage format for T x B ragged graphs (slot 0 = the observation the episode
starts from, slot t+1 = after action t):

    node_feat  [T+1, B, E, 7] f32          full rows every slot
    reward     [T+1, B, N]    f32          slot t+1: reward of action t
    cost       [T+1, B, N]    f32
    done       [T+1, B]       u8
    edge_count [T+1, B]       i32
    edge_ptr   [T+1, B+1]     i64          CSR offsets into the slot's edges
    edge_index [T+1, 2, cap]  i32          global node ids b*E + e
    edge_attr  [T+1, cap]     f32          distances
    actions    [T, B, N]      i32
    (assign    [T+1, B, N]    i32          ragged scenarios)

``cap`` is per slot (default 8 edges per entity per env, ~6x the mean at the
headline density); a slot whose ``edge_ptr[B]`` exceeds it has its edges
truncated (``overflowed()`` reports it), never written out of bounds.
``graph_batch`` assembles a PyG-style batch of (t, b) samples for the
minibatch generators; ``compute_returns`` is GAE over rewards or costs.
``graph_batch_csr`` assembles the same samples as the CSR batch (with its
transposed graph) the attention kernels take, in two HIP launches
(``gsm_graph_batch_ptr`` / ``gsm_graph_batch_gather``), and
``compute_returns(kernel=True)`` is the GAE loop as one launch (``gsm_gae``).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .batch import GpuBatchEnv


_ptr = _lib.ptr


class GraphRolloutBuffer:
    FIELDS = ("node_feat", "reward", "cost", "done", "edge_count", "edge_ptr", "edge_index", "edge_attr")

    def __init__(self, env: GpuBatchEnv, episode_length: Optional[int] = None,
                 edges_per_env: Optional[int] = None):
        self.env = env
        T = int(episode_length or env.cfg.episode_length)
        B, N, E = env.B, env.N, env.E
        per_env = int(edges_per_env or min(env.sizes.max_edges_per_env, 8 * E))
        cap = B * per_env
        dev = env.device
        f32, i32 = torch.float32, torch.int32
        self.T, self.B, self.N, self.E, self.cap = T, B, N, E, cap
        self.node_feat = torch.zeros(T + 1, B, E, 7, dtype=f32, device=dev)
        self.reward = torch.zeros(T + 1, B, N, dtype=f32, device=dev)
        self.cost = torch.zeros(T + 1, B, N, dtype=f32, device=dev)
        self.done = torch.zeros(T + 1, B, dtype=torch.uint8, device=dev)
        self.edge_count = torch.zeros(T + 1, B, dtype=i32, device=dev)
        self.edge_ptr = torch.zeros(T + 1, B + 1, dtype=torch.int64, device=dev)
        self.edge_index = torch.zeros(T + 1, 2, cap, dtype=i32, device=dev)
        self.edge_attr = torch.zeros(T + 1, cap, dtype=f32, device=dev)
        self.actions = torch.zeros(T, B, N, dtype=i32, device=dev)
        self.ragged = env.cfg.ragged
        if self.ragged:
            self.assign = torch.full((T + 1, B, N), -1, dtype=i32, device=dev)
        self.step = 0

    # ------------------------------------------------------------ storage
    def slot(self, t: int) -> dict:
        """The outputs of slot t as a dict of views (gsm_outputs for the env)."""
        d = {k: getattr(self, k)[t] for k in self.FIELDS}
        if self.ragged:
            d["assign"] = self.assign[t]
        return d

    @property
    def obs(self) -> torch.Tensor:
        """[T+1, B, N, 6] view: the agents' MPE observation (vel, pos, goal-rel)."""
        return self.node_feat[:, :, : self.N, :6]

    @property
    def rewards(self) -> torch.Tensor:
        return self.reward[1:]

    @property
    def costs(self) -> torch.Tensor:
        return self.cost[1:]

    @property
    def masks(self) -> torch.Tensor:
        """[T+1, B, N] f32: 0 after a step that ended the episode (MAPPO masks)."""
        m = 1.0 - self.done.to(torch.float32)
        m[0] = 1.0
        return m.unsqueeze(-1).expand(-1, -1, self.N)

    def overflowed(self) -> torch.Tensor:
        """Device bool: some slot had more edges than the per-slot capacity."""
        return (self.edge_ptr[:, self.B] > self.cap).any()

    # ------------------------------------------------------------ filling
    def reset(self, seed: Optional[int] = None) -> dict:
        """Reset the env and write the first observation into slot 0."""
        self.env.reset(seed=seed, sync_edges=False)
        self.step = 0
        return self.env.observe(out=self.slot(0))

    def insert(self, actions: torch.Tensor) -> dict:
        """env.step(actions) writing straight into the next slot."""
        if self.step >= self.T:
            raise IndexError("buffer is full; call after_update()")
        out = self.env.step(actions, out=self.slot(self.step + 1))
        if actions.dtype == torch.int32:
            self.actions[self.step].copy_(actions)
        elif actions.shape[-1] == 5:          # one-hot: store the index
            self.actions[self.step].copy_(actions.argmax(-1))
        # continuous actions are not stored (the buffer keeps discrete indices)
        self.step += 1
        return out

    def capture(self, actions_seq: torch.Tensor, slot: int = 0) -> None:
        """One HIP graph that steps the whole episode from the env's current
        state, step j writing slot j+1 (actions_seq: int32 [T, B, N])."""
        self.env.capture_into(actions_seq, [self.slot(t + 1) for t in range(self.T)], slot=slot)
        self._graph_actions = actions_seq

    def replay(self, slot: int = 0) -> None:
        """Run a captured episode; slot 0 must already hold its first observation.
        The episode usually runs as one fused rollout launch, whose bounded
        in-launch waits can (in principle) time out and leave invalid edges:
        the next read of the buffer (``graph_batch``, ``validate``) checks."""
        self.env.replay(slot)
        n = self._graph_actions.shape[0]
        idx = torch.arange(self.T, device=self._graph_actions.device) % n
        self.actions.copy_(self._graph_actions[idx])
        self.step = self.T
        self._unchecked = True

    def validate(self) -> None:
        """Raise if a replayed episode's launch gave up a bounded wait (its
        CSR offsets and edges would be wrong). Synchronises; a no-op when no
        replay happened since the last check."""
        if getattr(self, "_unchecked", False):
            self._unchecked = False
            if self.env.roll_gave_up():
                raise RuntimeError("GraphRolloutBuffer: a fused rollout launch gave up waiting on a "
                                   "predecessor workgroup; the episode's edges are invalid")

    def after_update(self) -> None:
        """Carry the last observation into slot 0 for the next rollout."""
        self.validate()
        for k in self.FIELDS + (("assign",) if self.ragged else ()):
            buf = getattr(self, k)
            buf[0].copy_(buf[self.step])
        self.step = 0

    # ------------------------------------------------------------- reading
    def graph_batch(self, t_idx: torch.Tensor, b_idx: torch.Tensor) -> dict:
        """PyG-style batch of K samples (slot t_idx[k], env b_idx[k]): node_feat
        [K*E, 7], edge_index [2, sum] int64 with local ids k*E + e, edge_attr,
        batch [K*E] (sample of each node), ptr [K+1] (edge offsets).
        Raises ValueError if a requested sample's edges were truncated because
        its slot overflowed the per-slot edge capacity (``overflowed()``), and
        RuntimeError if the replayed episode's launch gave up a bounded wait."""
        self.validate()
        E = self.E
        t = t_idx.to(self.edge_ptr.device, torch.int64)
        b = b_idx.to(self.edge_ptr.device, torch.int64)
        K = t.numel()
        start = self.edge_ptr[t, b]
        end = self.edge_ptr[t, b + 1]
        if bool((end > self.cap).any()):
            raise ValueError(f"graph_batch: a requested sample's edges run past the slot capacity {self.cap} "
                             "(the slot overflowed and was truncated); size the buffer with a larger edge "
                             "capacity")
        cnt = end - start
        ptr = torch.zeros(K + 1, dtype=torch.int64, device=t.device)
        torch.cumsum(cnt, 0, out=ptr[1:])
        total = int(ptr[-1].item())
        k = torch.repeat_interleave(torch.arange(K, device=t.device), cnt, output_size=total)
        j = start[k] + (torch.arange(total, device=t.device) - ptr[k])
        tk = t[k]
        src = self.edge_index[tk, 0, j].to(torch.int64)
        dst = self.edge_index[tk, 1, j].to(torch.int64)
        shift = (k - b[k]) * E          # global id b*E + e  ->  local id k*E + e
        return dict(node_feat=self.node_feat[t, b].reshape(K * E, 7),
                    edge_index=torch.stack([src + shift, dst + shift]),
                    edge_attr=self.edge_attr[tk, j],
                    batch=torch.arange(K, device=t.device).repeat_interleave(E),
                    ptr=ptr)

    def graph_batch_csr(self, t_idx: torch.Tensor, b_idx: torch.Tensor, transpose: bool = True,
                        check: bool = True) -> dict:
        """The samples of ``graph_batch`` as the CSR batch the attention kernels
        take, assembled by two HIP launches (gsm_graph_batch_ptr,
        gsm_graph_batch_gather): node_feat [K*E, 7], row_ptr int64 [K*E+1], col
        int32 [sum] (local ids k*E + e), edge_attr [sum], ptr [K+1] (the
        samples' entry offsets), status (device int32 [1], GSM_BATCH_* bits) and
        ``transpose`` = (row_ptr, t_edge, col), the transposed graph for
        ``attn_aggregate_autograd`` / ``TransformerConv.forward(transpose=...)``
        (None with ``transpose=False``): ``gnn.csr_transpose`` of the batch
        without its sort, since the env's graphs are symmetric with ascending
        rows and columns. One host synchronisation reads the entry total that
        sizes the outputs, and with it the first launch's status: IndexError for
        an out-of-range index, ValueError for a sample whose slot overflowed
        the edge capacity. With ``check`` a second one reads the gather's status
        (RuntimeError for an entry outside its env or without its reverse
        entry); without, the caller has ``status``."""
        self.validate()
        E, dev = self.E, self.edge_ptr.device
        t = t_idx.to(dev, torch.int64).contiguous()
        b = b_idx.to(dev, torch.int64).contiguous()
        K = t.numel()
        if b.numel() != K:
            raise ValueError("graph_batch_csr: t_idx and b_idx differ in length")
        i32, i64 = torch.int32, torch.int64
        if K == 0:
            row_ptr, col = torch.zeros(1, dtype=i64, device=dev), torch.zeros(0, dtype=i32, device=dev)
            return dict(node_feat=self.node_feat.new_zeros(0, 7), row_ptr=row_ptr, col=col,
                        edge_attr=self.edge_attr.new_zeros(0), ptr=torch.zeros(1, dtype=i64, device=dev),
                        transpose=(row_ptr, torch.zeros(0, dtype=i32, device=dev), col) if transpose else None,
                        status=torch.zeros(1, dtype=i32, device=dev))
        lib = _lib.load()
        S, B = self.T + 1, self.B
        stream = _lib.stream(dev)
        # sample offsets [K+1] and the status word in one allocation: its last
        # two words come back in one copy
        head = torch.zeros(K + 2, dtype=i64, device=dev)
        ptr, status = head[:K + 1], head[K + 1:].view(i32)[:1]
        _lib.check(lib, lib.gsm_graph_batch_ptr(_ptr(self.edge_ptr), S, B, self.cap, _ptr(t), _ptr(b), K, _ptr(ptr),
                                                _ptr(status), stream), None, "gsm_graph_batch_ptr")
        total, st = head[K:].cpu().tolist()
        st &= 0xFFFFFFFF
        if st & _lib.BATCH_BAD_INDEX:
            raise IndexError(f"graph_batch_csr: a sample's slot is outside [0, {S}) or its env outside [0, {B})")
        if st & _lib.BATCH_TRUNCATED:
            raise ValueError(f"graph_batch_csr: a requested sample's edges run past the slot capacity {self.cap} "
                             "(the slot overflowed and was truncated); size the buffer with a larger edge "
                             "capacity")
        if st:
            raise RuntimeError("graph_batch_csr: a requested sample's edge offsets are corrupt (end < start)")
        if total >= 2 ** 31 or K * E >= 2 ** 31:
            raise ValueError("graph_batch_csr: the batch needs fewer than 2^31 nodes and entries")
        node_feat = torch.empty(K * E, 7, dtype=torch.float32, device=dev)
        row_ptr = torch.empty(K * E + 1, dtype=i64, device=dev)
        col = torch.empty(total, dtype=i32, device=dev)
        edge_attr = torch.empty(total, dtype=torch.float32, device=dev)
        t_edge = torch.empty(total, dtype=i32, device=dev) if transpose else None
        rc = lib.gsm_graph_batch_gather(_ptr(self.node_feat), _ptr(self.edge_index), _ptr(self.edge_attr),
                                        _ptr(self.edge_ptr), S, B, E, self.cap, _ptr(t), _ptr(b), _ptr(ptr), K, total,
                                        _ptr(node_feat), _ptr(row_ptr), _ptr(col), _ptr(edge_attr), _ptr(t_edge),
                                        _ptr(status), stream)
        _lib.check(lib, rc, None, "gsm_graph_batch_gather")
        if check:
            st = int(status.item())
            if st:
                what = [w for bit, w in ((_lib.BATCH_OUT_OF_ENV, "an entry's node id lies outside its env"),
                                         (_lib.BATCH_ASYMMETRIC, "an entry's reverse entry is missing (the graph "
                                                                 "is not symmetric with ascending columns)"),
                                         (_lib.BATCH_BAD_OFFSETS, "the sample offsets do not match the slots"))
                        if st & bit]
                raise RuntimeError(f"graph_batch_csr: the stored graph is invalid (status {st}): " + "; ".join(what))
        return dict(node_feat=node_feat, row_ptr=row_ptr, col=col, edge_attr=edge_attr, ptr=ptr,
                    transpose=(row_ptr, t_edge, col) if transpose else None, status=status)

    def render(self, env: int = 0, slots=None, width: int = 700, height: int = 700,
               edges: bool = True) -> torch.Tensor:
        """Frames uint8 [len(slots), H, W, 3] of env ``env`` over the stored
        slots (default: all T+1), straight from the buffer (gsmarl_amd.render);
        ``gsmarl_amd.render.save_gif`` writes them out."""
        from .render import render_frames
        c = self.env.cfg
        slots = range(self.T + 1) if slots is None else slots
        frames = [render_frames(self.node_feat[t], self.edge_ptr[t], self.edge_index[t], [env], width, height,
                                (c.agent_size, c.goal_size, c.obstacle_size), c.world_half or 0.0, edges)
                  for t in slots]
        return torch.cat(frames)

    def compute_returns(self, values: torch.Tensor, gamma: float = 0.99, gae_lambda: float = 0.95,
                        which: str = "reward", kernel: bool = False) -> torch.Tensor:
        """GAE returns [T, B, N] of the rewards (or costs, for the safe-RL
        cost critic) given value predictions values [T+1, B, N]. With
        ``kernel`` the loop below runs as one HIP launch (gsm_gae), bit for bit
        the same returns."""
        r = self.rewards if which == "reward" else self.costs
        if kernel:
            if values.shape != (self.T + 1, self.B, self.N) or values.device != r.device:
                raise ValueError(f"values: need [{self.T + 1}, {self.B}, {self.N}] on {r.device}")
            v = values.to(torch.float32).contiguous()
            ret = torch.empty_like(r)
            lib = _lib.load()
            stream = _lib.stream(r.device)
            # gamma * gae_lambda: the double product, rounded once to fp32 as the loop's scalar is
            rc = lib.gsm_gae(_ptr(r), _ptr(v), _ptr(self.done), self.T, self.B, self.N, float(gamma),
                             float(gamma * gae_lambda), _ptr(ret), stream)
            _lib.check(lib, rc, None, "gsm_gae")
            return ret
        masks = self.masks
        ret = torch.empty_like(r)
        gae = torch.zeros_like(r[0])
        for t in reversed(range(self.T)):
            delta = r[t] + gamma * values[t + 1] * masks[t + 1] - values[t]
            gae = delta + gamma * gae_lambda * masks[t + 1] * gae
            ret[t] = gae + values[t]
        return ret
