"""hipGraph capture of the replay-sample -> Bellman-update step.

One step is ~30 kernel launches on two HIP streams; launched eagerly the host spends ~380 us per step on
launch API calls, about as long as the GPU needs to run them.  ``GraphedUpdate`` captures `S` consecutive
steps (index rows -> [sum-tree query] -> row gather -> learn_on_batch -> [priority write-back]) once, with
static buffers, and replays them: one graph launch per S steps.

The draws stay on the host (numpy PCG64, the reference's stream): before a replay the next S rows of
pre-drawn dense indices (uniform) or unit draws (prioritized) are copied into the static input block; so are the betas of a weighted
update and the (horizon, discount) pairs of one under a horizon schedule, which the kernels read from device memory.
"""
from __future__ import annotations

import numpy as np
import torch

from slimdqn import _hip


class GraphedUpdate:
    def __init__(self, rb, eng, prioritized: bool, steps_per_graph: int = 8, writeback: bool | None = None, learn=None,
                 weighted: bool = False, augment=None, state=(), horizon: bool = False):
        """``prioritized``: the sampler is a sum tree (the query is part of the graph); ``writeback``: sqrt(mean_k td) of
        every step goes back into the tree (default: whenever prioritized); ``learn``: the learn call of one step on a C batch
        (default ``eng.learn_on_batch``; DQN passes its target-parameter form, dqn.py:59-72); ``weighted``: the query also writes
        the importance-sampling weights of its draws and the learn call applies them (prioritized only).  The betas are INPUT of
        a replay, like the draws: ``run(betas)`` stages one per step, the query kernel reads its step's from device memory -- a
        replay with other betas is the same executable graph.  ``augment``: (pad, seed, device counter) of the random-shift augmentation
        (include/isdqn_hip.h, isdqn_replay_augment_shift) or None -- the gathered rows' frames are shifted into a scratch pool inside the
        graph and every step's batch reads the pool; the counter lives on the device, so every replay draws anew and lands on the
        draws the eager steps would have taken.  ``state``: device tensors besides the engine's own that ``learn`` writes (DQN with
        ``ema_tau``: the target buffers) -- the warm-up steps of a capture must not count on them either.  ``horizon``: the replay keeps
        horizon windows and every step's rows are cut at a horizon and discount of its own (include/isdqn_hip.h,
        isdqn_replay_gather_horizon); the S pairs are INPUT of a replay, like the betas -- ``run(betas, horizons, gammas)`` stages them,
        the gather of step s reads its pair from device memory, and the step's batch carries the gathered discounts."""
        self.horizon = bool(horizon)
        if self.horizon and not getattr(rb, "_horizon_window", False):
            raise ValueError("a captured update at a horizon needs a replay built with horizon_window=True")
        self.augment = augment
        self._learn_state = list(state)
        self.augment_pad = int(augment[0]) if augment else 0
        if weighted and not prioritized:
            raise ValueError("importance-sampling weights need the prioritized sampling distribution")
        self.rb, self.eng, self.prioritized, self.S = rb, eng, prioritized, steps_per_graph
        self.weighted = bool(weighted)
        self._learn = eng.learn_on_batch if learn is None else learn
        self.writeback = prioritized if writeback is None else (writeback and prioritized)
        dev, B, s2 = eng.device, eng.batch_size, 2 * rb._stack_size
        self.B = B
        rb._flush()
        self.block = torch.zeros(self.S, B, dtype=torch.float64 if prioritized else torch.int32, device=dev)
        self.indices = torch.zeros(B, dtype=torch.int32, device=dev)
        # Uniform sampling: the S steps of a replay sample an unchanged buffer with indices drawn beforehand, so their S
        # row gathers are ONE launch over S*B rows at the head of the graph (one 6 us kernel at the head of a step
        # less); every step then has its own static batch.  Prioritized sampling depends on the previous step's
        # priority write-back and keeps one gather per step into a single batch.
        # Prioritized: two batch slots alternate, because the write-back of step s and the draw + gather of step s+1 run on a
        # second stream under the backward pass of step s (learn_on_batch records `priorities_ready` for it).
        n_b = 2 if prioritized else self.S
        if prioritized:
            self.indices = torch.zeros(2, B, dtype=torch.int32, device=dev)
            self._sampling_stream = torch.cuda.Stream(dev)
            self._prio_ready = [torch.cuda.Event() for _ in range(2)]
            for e in self._prio_ready:
                e.record(self._sampling_stream)  # creates the handle the C ABI takes
        # weights of the two batch slots (the query of slot 1 - slot writes them on the sampling stream) and the S betas
        self.weights = torch.ones(2, B, dtype=torch.float32, device=dev) if self.weighted else None
        self.betas = torch.zeros(self.S, dtype=torch.float32, device=dev) if self.weighted else None
        self.frame_ids = torch.zeros(n_b, B, s2, dtype=torch.int32, device=dev)
        self.action = torch.zeros(n_b, B, dtype=torch.int32, device=dev)
        self.reward = torch.zeros(n_b, B, dtype=torch.float32, device=dev)
        self.terminal = torch.zeros(n_b, B, dtype=torch.uint8, device=dev)
        # the pairs of the S steps (horizon 1, discount 0 until run() stages them: the warm-up of a capture reads them) and the
        # gathered discounts of every batch slot
        self.horizons = torch.ones(self.S, dtype=torch.int32, device=dev) if self.horizon else None
        self.gammas = torch.zeros(self.S, dtype=torch.float32, device=dev) if self.horizon else None
        self.discount = torch.zeros(n_b, B, dtype=torch.float32, device=dev) if self.horizon else None
        # vector observations (the fc torso, LunarLander): the replay stores the bytes of every float32 observation as one 1 x 4d "frame";
        # the captured step materialises the B state / next-state rows of a batch into static buffers the engine reads as (B, d) float32
        self.fc = eng.architecture_type == "fc"
        if self.augment:
            if self.fc:
                raise ValueError("random-shift augmentation shifts image frames: not with the fc torso")
            # uniform: one pool over the S*B rows of a replay (one launch behind the single gather, rows_per_step = B); prioritized: one
            # pool per batch slot, filled behind that slot's gather on the stream that gathered
            self.aug_frames = torch.zeros(n_b, B * s2, rb._hw, dtype=torch.uint8, device=dev)
            self.aug_ids = torch.full((n_b, B, s2), -1, dtype=torch.int32, device=dev)
        if self.fc:
            if not rb._obs_float or rb._stack_size != 1:
                raise NotImplementedError("captured fc step: float32 vector observations with stack_size 1")
            self.obs = torch.zeros(2, n_b * B, rb._w, dtype=torch.uint8, device=dev)  # [state | next_state][slot * B + b][4 d]
        self._frames_ptr = rb._frames.data_ptr()
        self._make_batches()
        # Every captured step takes the weight mirror as it is; run() rebuilds it in front of the replay (one eager 8 us launch) only
        # when the engine's bookkeeping says something wrote the parameters since the last call that left it current (consecutive
        # replays and acting in between do not: _engine.py _mirror_is_current).  (A second capture that rebuilds at its head was the
        # first form of this; it crashed hipGraphLaunch in hip::Graph::UpdateStreams in some test orders.  Cause, DESIGN.md
        # "hipGraphLaunch fault": at launch the runtime fills the graph's stream array from the executable's own pool of
        # parallel streams, skips every pool stream that maps to the launch stream's queue, and indexes the pool WITHOUT a bound:
        # one skipped entry too many and it reads a Stream* past the end of the vector.  Which pool stream aliases the launch
        # stream depends on how many streams the process created before the instantiation -- the test order.  The agents therefore
        # keep ONE live executable each, destroy it before capturing a successor, and never re-instantiate in steady state.)
        self.graph = None
        self._capture()
        if getattr(eng, "_captured", None) is None:  # (the engine drops its captured updates when an option that travels in the batches changes)
            import weakref

            eng._captured = weakref.WeakSet()
        eng._captured.add(self)

    def destroy(self) -> None:
        """Release the executable graph (and the runtime's parallel streams it owns) after everything it enqueued has finished.
        An agent calls this on the update object it replaces BEFORE it captures the successor."""
        if self.graph is not None:
            torch.cuda.synchronize(self.eng.device)
            self.graph.reset()
            self.graph = None

    def _make_batches(self) -> None:
        rb, eng = self.rb, self.eng
        # every step of a replay finds the weight mirror current: steps 2..S follow a learn step of the same graph, step 1 follows
        # run()'s check
        ev = lambda i: self._prio_ready[i] if self.prioritized else None
        wt = lambda i: self.weights[i] if self.weighted else None
        dc = lambda i: self.discount[i] if self.horizon else None
        if self.fc:
            B = self.B
            rows = lambda half, i: self.obs[half, i * B:(i + 1) * B].view(torch.float32)
            self.chained = [
                eng.make_batch(state=rows(0, i), next_state=rows(1, i), action=self.action[i], reward=self.reward[i], terminal=self.terminal[i],
                               mirror_current=True, priorities_ready=ev(i), loss_weights=wt(i), discount=dc(i))
                for i in range(self.frame_ids.shape[0])
            ]
            return
        # augmented: the batch reads the scratch pool through the table into it -- the one pool of the S*B-row launch (uniform: the ids
        # of step i count from the pool's base), or the slot's own (prioritized)
        if self.augment:
            frames = lambda i: self.aug_frames[i] if self.prioritized else self.aug_frames
            ids = lambda i: self.aug_ids[i]
        else:
            frames = lambda i: rb._frames
            ids = lambda i: self.frame_ids[i]
        self.chained = [
            eng.make_batch(frames=frames(i), frame_stride=rb._hw, frame_ids=ids(i), action=self.action[i],
                           reward=self.reward[i], terminal=self.terminal[i], mirror_current=True, priorities_ready=ev(i),
                           loss_weights=wt(i), discount=dc(i))
            for i in range(self.frame_ids.shape[0])
        ]

    def _gather(self, idx, n_rows: int, slot: int, s: int = 0) -> None:
        """Rows of ``idx`` into the batch buffers from slot ``slot`` on; with horizon windows, the B rows of step ``s`` at its pair."""
        rb = self.rb
        if self.horizon:
            assert n_rows == self.B
            rb.gather_horizon_into(idx, self.horizons[s:s + 1], self.gammas[s:s + 1], self.frame_ids[slot], self.action[slot],
                                   self.reward[slot], self.terminal[slot], self.discount[slot])
            return
        _hip.check(
            rb._lib.isdqn_replay_gather_rows(
                _hip.ptr(rb._d_elem_frames), _hip.ptr(rb._d_elem_action), _hip.ptr(rb._d_elem_reward),
                _hip.ptr(rb._d_elem_terminal), rb._stack_size, _hip.ptr(rb._d_index_to_slot), _hip.ptr(idx), n_rows,
                _hip.ptr(self.frame_ids[slot]), _hip.ptr(self.action[slot]), _hip.ptr(self.reward[slot]),
                _hip.ptr(self.terminal[slot]), _hip.stream_ptr(self.eng.device),
            ),
            "isdqn_replay_gather_rows",
        )

    def _augment(self, slot: int, n_rows: int) -> None:
        """Shift the frames of ``n_rows`` gathered rows, from batch slot ``slot`` on, into the pool (current stream); nothing when off."""
        if self.augment:
            pad, seed, count = self.augment
            self.rb.augment_into(self.frame_ids[slot], n_rows, self.B, pad, seed, count, self.aug_frames[slot], self.aug_ids[slot])

    def _materialize(self, slot: int, n_rows: int) -> None:
        """fc: the observation rows of ``n_rows`` gathered transitions, from batch slot ``slot`` on."""
        rb, B = self.rb, self.B
        _hip.check(
            rb._lib.isdqn_replay_materialize(
                _hip.ptr(rb._frames), rb._hw, rb._h, rb._w, rb._stack_size, _hip.ptr(self.frame_ids[slot]), n_rows,
                _hip.ptr(self.obs[0, slot * B:]), _hip.ptr(self.obs[1, slot * B:]), _hip.stream_ptr(self.eng.device),
            ),
            "isdqn_replay_materialize",
        )

    def _query(self, tree, s: int, slot: int) -> None:
        """Draw of step ``s`` into batch slot ``slot`` (weighted: its importance-sampling weights with it, one launch)."""
        if self.weighted:
            tree.query_device(self.block[s], out=self.indices[slot], unit=True, beta=self.betas[s:s + 1], weights_out=self.weights[slot])
        else:
            tree.query_device(self.block[s], out=self.indices[slot], unit=True)

    def _steps(self) -> None:
        """The S steps of one replay, enqueued on the current stream.  The first node rebuilds the weight mirror from the parameters
        as they are when the replay starts (whoever wrote them, however: _engine.py "weight-mirror bookkeeping"); the steps behind
        it trust it -- each follows a learn step of the same replay, whose optimizer wrote both forms."""
        rb, eng = self.rb, self.eng
        if not eng.trust_mirror:
            eng.rebuild_mirror()
        if self.prioritized:
            tree = rb._sampling_distribution._sum_tree
            main, sampling = torch.cuda.current_stream(eng.device), self._sampling_stream
            self._query(tree, 0, 0)
            self._gather(self.indices[0], self.B, 0)
            self._augment(0, self.B)
            for s in range(self.S):
                slot = s & 1
                if self.fc:
                    self._materialize(slot, self.B)
                self._learn(self.chained[slot])
                # under the rest of this step (backward, Adam): priorities of step s into the tree, then the draw and the row
                # gather of step s+1 -- the order the reference's loop has (update, then sample)
                sampling.wait_event(self._prio_ready[slot])
                with torch.cuda.stream(sampling):
                    if self.writeback:
                        rb._sampling_distribution.update_device(self.indices[slot], eng.priorities)
                    if s + 1 < self.S:
                        self._query(tree, s + 1, 1 - slot)
                        self._gather(self.indices[1 - slot], self.B, 1 - slot, s + 1)
                        self._augment(1 - slot, self.B)
                main.wait_stream(sampling)
        else:
            if self.horizon:  # (every step has a horizon of its own: S gathers of B rows in place of the one over S*B)
                for s in range(self.S):
                    self._gather(self.block[s], self.B, s, s)
            else:
                self._gather(self.block, self.S * self.B, 0)  # rows of all S steps: the [S][B] buffers are contiguous
            self._augment(0, self.S * self.B)  # (and so are the pool and its table: step s takes the draws of count + s)
            if self.fc:
                self._materialize(0, self.S * self.B)
            for s in range(self.S):
                self._learn(self.chained[s])

    def _capture(self) -> None:
        # warm-up on a side stream (lazy one-time setup inside the library must not happen during capture)
        side = torch.cuda.Stream(self.eng.device)
        side.wait_stream(torch.cuda.current_stream(self.eng.device))
        # (with gradient clipping the warm-up steps also add to the gradient-norm accumulators, region "grad_clip"[2:4])
        training = [self.eng.params, self.eng.adam_m, self.eng.adam_v, self.eng.adam_count, self.eng.losses_accum]
        if getattr(self.eng, "max_grad_norm", 0.0) > 0.0:
            training.append(self.eng.grad_clip[2:4])
        # (noisy engines: every captured step holds the resample -- the device counter makes each replay draw anew -- and the noisy
        # learn; the warm-up's draws and sigma updates must not count either)
        if getattr(self.eng, "noisy", False):
            training += [self.eng.sigma, self.eng.sigma_m, self.eng.sigma_v, self.eng.noise_count]
        if self.augment:  # (the warm-up's draws must not count: the captured steps take the draws the eager steps would)
            training.append(self.augment[2])
        training += self._learn_state
        state = [t.clone() for t in training]
        # (prioritized: the warm-up also writes priorities back -- with the zero-filled draw block -- so the whole tree
        # state is saved: nodes, max_recorded_priority, which every later add() reads, and the latched status word)
        tree = self.rb._sampling_distribution._sum_tree if self.prioritized else None
        tree_state = [t.clone() for t in (tree._nodes_dev, tree._max_dev, tree._status)] if tree is not None else None
        with torch.cuda.stream(side):
            self.eng.rebuild_mirror()
            self._steps()
        torch.cuda.current_stream(self.eng.device).wait_stream(side)
        torch.cuda.synchronize(self.eng.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._steps()
        # the warm-up steps must not count: restore the training state
        for dst, src in zip(training, state):
            dst.copy_(src)
        if tree is not None:
            for dst, src in zip((tree._nodes_dev, tree._max_dev, tree._status), tree_state):
                dst.copy_(src)
        # the restored parameters are not what the warm-up's optimizer left in the mirror
        self.eng.invalidate_mirror()
        self.graph = g

    def run(self, betas=None, horizons=None, gammas=None) -> None:
        """S steps: draw S index rows on the host stream of the sampler, stage them (weighted: and the S float32 ``betas`` of these
        steps; at a horizon: and their S int32 ``horizons`` and float32 ``gammas``), replay the graph."""
        rb = self.rb
        if self.weighted != (betas is not None):
            raise ValueError("a weighted captured update takes the betas of its S steps, an unweighted one none")
        if self.horizon != (horizons is not None) or self.horizon != (gammas is not None):
            raise ValueError("a captured update at a horizon takes the horizons and the gammas of its S steps, another one neither")
        rb._flush()
        # the frame store was re-allocated: pointers in the graph are stale; or the engine dropped the graph (set_weight_decay)
        if rb._frames.data_ptr() != self._frames_ptr or self.graph is None:
            self._frames_ptr = rb._frames.data_ptr()
            self.destroy()
            self._make_batches()
            self._capture()
        sampler = rb._sampling_distribution
        rows = sampler.draw_rows_device(self.S, self.B)
        self.block.copy_(rows, non_blocking=True)
        if self.weighted:
            betas = np.ascontiguousarray(betas, dtype=np.float32)
            assert betas.shape == (self.S,)
            self.betas.copy_(sampler._to_device(betas, torch.float32), non_blocking=True)
        if self.horizon:
            horizons = np.ascontiguousarray(horizons, dtype=np.int32)
            gammas = np.ascontiguousarray(gammas, dtype=np.float32)
            assert horizons.shape == (self.S,) and gammas.shape == (self.S,)
            self.horizons.copy_(sampler._to_device(horizons, torch.int32), non_blocking=True)
            self.gammas.copy_(sampler._to_device(gammas, torch.float32), non_blocking=True)
        if self.eng.trust_mirror:
            self.eng.refresh_mirror()  # (trusted engines only: one eager launch when the bookkeeping says the mirror is stale)
        self.graph.replay()
        if getattr(self.eng, "noisy", False):
            self.eng.invalidate_mirror()  # (the mirror holds the last step's composed parameters, not mu)
            self.eng._noise_zero = False
        else:
            self.eng._mirror_made_current()  # the last step's optimizer wrote both forms of the weights
