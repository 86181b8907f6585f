"""ClosedLoopMPC: receding-horizon control with the step between two ticks on the GPU.

One tick = DeviceSQPOptimizationSolver.getOptimalSolution (evaluate, solve, step, merit: every layer a kernel) followed by one
mpcqp_stage_advance kernel (StageEvaluator.advance): the plant step by the model's own discrete map (or a measured state), the trajectory,
the QP start, the ADMM duals and the per-frame references shifted by one stage, and the new first frame pinned in lbx / ubx as
computeOptimalTrajectory pins it on the host (reference src/OptimalControlProblem.cpp:93-96).  The iterate, the bounds, the duals and the plant
state never leave the device; x, dw, y and p are double-buffered because the shift is out of place.

shift=False keeps the reference's hand-over for comparison: result_ persists (SQPOptimizationSolver.cpp:88-91, OptimalControlProblem.cpp:113), so
the next tick starts from the previous trajectory unshifted and the duals of stage k are offered to stage k; only the first frame is re-pinned.
The references still move by one frame per tick -- they are data about the world, not a warm start -- and so do the stage data (set_stage_data)."""
import numpy as np

from .sqp import DeviceSQPOptimizationSolver


class ClosedLoopMPC:
    def __init__(self, model, options=None, batch=1, tail="rollout", shift=True, device=-1, codegen=None, shift_data=True, feedback=None, soft_rows=None):
        """model: a models.StageOCP (zoo, generated or per_frame_reference).  options: those of DeviceSQPOptimizationSolver, passed through
        (warm_start_admm, carry_rho, constant_matrices, keep_scaling, presolve_fixed_rows, ...); max_iter defaults to 1 SQP iteration per
        tick and alpha to 1 (real-time iteration), skip_failed_steps to True (an infeasible QP keeps its iterate and holds the input).
        options["direct_qp"]: a tick's QP is first solved directly where no inequality is active; the hand-over takes the merged
        dw, y and status, and sol.direct_history holds the verdicts per tick.  With its "active_set" key the set of held inputs a tick
        ends with (sol.act) is shifted by one frame with the plan -- a device slice copy, the last frame repeats -- and is the next tick's guess.
        With its "interior_point" key the QPs whose plans ride state bounds are solved directly as well; nothing is carried between ticks,
        and sol.direct_iters_history holds the iteration counts per tick.
        shift_data=False: a tick does not shift the stored stage data -- rows that belong to horizon positions, not to world time (the step
        lengths of a non-uniform time grid, models.StageOCP.transition_data); tick's d_new is then a ValueError.
        feedback=True or {"clamp_tol": ..., "reg": ...}: every tick also computes the time-varying LQR gains around its plan (one
        mpcqp_stage_riccati on the tick's local system; K, gain_failed) and hold() becomes available -- a plant step without a solve that tracks
        the plan with u = u_k + K_k (s - s_k).  Without the option a tick is what it was, not a launch more.
        soft_rows: options["soft_rows"] of the loop (a dict for models.StageOCP.soft_rows, or (w1, w2) over the rows): a measured state outside its
        box no longer makes the tick's QP infeasible.  The weights belong to horizon positions and are not shifted."""
        import torch
        if feedback is not None and feedback is not True and not isinstance(feedback, dict):
            raise ValueError("feedback: expected None, True or a dict with clamp_tol and / or reg")
        fb = {} if feedback is True else feedback
        if fb is not None:
            unknown = set(fb) - {"clamp_tol", "reg"}
            if unknown:
                raise ValueError("feedback: unknown keys %s (clamp_tol and reg are the options)" % sorted(unknown))
            if not (float(fb.get("clamp_tol", 0.0)) >= 0.0) or not (float(fb.get("reg", 0.0)) >= 0.0):
                raise ValueError("feedback: clamp_tol and reg must not be negative")
            if getattr(model, "link_cost", False):
                raise ValueError("feedback: this model has a link cost: its Hessian couples neighbouring frames, and the Riccati sweep over the frame "
                                 "blocks alone would drop those terms")
            fb = {"clamp_tol": float(fb.get("clamp_tol", 0.0)), "reg": float(fb.get("reg", 0.0))}
        self.feedback = fb
        if tail not in ("repeat", "rollout"):
            raise ValueError("tail must be 'repeat' or 'rollout'")
        opts = dict(options or {})
        if soft_rows is not None:
            if opts.get("soft_rows") is not None:
                raise ValueError('soft_rows: given both as an argument and as options["soft_rows"]')
            opts["soft_rows"] = soft_rows
        if opts.get("exact_hessian"):
            raise ValueError("exact_hessian is not available in ClosedLoopMPC: the multiplier estimate would need its own shift in advance, and "
                             "running a tick with unshifted multipliers would be silently wrong")
        opts.setdefault("max_iter", 1); opts.setdefault("alpha", 1.0); opts.setdefault("skip_failed_steps", True)
        self.model, self.batch, self.tail, self.shift, self.shift_data = model, int(batch), tail, bool(shift), bool(shift_data)
        self.sol = DeviceSQPOptimizationSolver(model, opts, batch=self.batch, device=device, codegen=codegen)
        self.ev, self.dev = self.sol.ev, self.sol.dev
        ev = self.ev
        mk = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=self.dev)
        B = self.batch
        self._x2 = mk(B, ev.nvar); self._dw2 = mk(B, ev.n); self._y2 = mk(B, ev.m)
        self.p = mk(B, ev.np); self._p2 = mk(B, ev.np) if ev.per_frame_reference else None
        self.lbx = mk(B, ev.nvar); self.ubx = mk(B, ev.nvar); self.lbg = mk(B, ev.ng); self.ubg = mk(B, ev.ng)
        self.applied = mk(B, ev.nx + ev.nu); self.stage_cost = mk(B)
        self._act2 = torch.zeros_like(self.sol.act) if self.sol.direct_active is not None else None
        self.ticks = 0
        self._ready = False
        self._has_data = False
        self.rollout_diverged = None; self.rollout_box_viol = None
        # feedback: the gains of the last tick's plan, the frame that failed per instance, the inputs' correction of the last hold, the holds since
        self.age = 0
        if self.feedback is not None:
            self.K = mk(B, ev.horizon, ev.nu, ev.nx)
            self.gain_failed = torch.full((B,), -1, dtype=torch.int32, device=self.dev)
            self.du = mk(B, ev.nu)
            self.plan = mk(B, ev.nvar)

    def reset(self, frame0, reference=None, x0=None):
        """frame0 [B, f] (or [f]): the measured state and the input being applied, pinned as the first frame.  reference: p, [B, nx] -- or
        [B, N nx] / [B, N, nx] for a per_frame_reference model -- zero when omitted.  x0: the iterate to start from; zero like the reference's.
        x0 = "rollout": the trajectory of the pinned first frame under its input held (one mpcqp_stage_rollout on the bounds just written, so the
        first tick linearises about a dynamically feasible trajectory); x0 = "reshoot": the same with zero inputs clipped to the box.
        rollout_diverged / rollout_box_viol (device tensors) report the outcome."""
        import torch
        m, B = self.model, self.batch
        shoot = {"rollout": "hold", "reshoot": "iterate"}.get(x0) if isinstance(x0, str) else None
        if isinstance(x0, str) and shoot is None:
            raise ValueError("x0: expected an iterate, None, 'rollout' or 'reshoot'")
        if shoot is not None:
            x0 = None
        f0 = np.broadcast_to(np.asarray(frame0, float).reshape(-1, m.f), (B, m.f))
        for t, v in zip((self.lbx, self.ubx, self.lbg, self.ubg), m.stacked_bounds(f0)):
            t.copy_(torch.as_tensor(v, dtype=torch.float64))
        ref = np.zeros((B, m.np)) if reference is None else np.broadcast_to(np.asarray(reference, float).reshape(-1, m.np), (B, m.np))
        self.p.copy_(torch.as_tensor(np.array(ref), dtype=torch.float64))
        self.sol.setInitialGuess(np.zeros(self.ev.nvar) if x0 is None else x0)
        if shoot is not None:      # the bounds are written: the first frame of the zero iterate is clipped onto the pinned one
            r = self.ev.rollout(self.sol.x, lbx=self.lbx, ubx=self.ubx, inputs=shoot, stream=torch.cuda.current_stream(self.dev).cuda_stream)
            self.rollout_diverged, self.rollout_box_viol = r["diverged"], r["box_viol"]
        if self.sol.direct_active is not None:
            self.sol.act.zero_()      # no guess from an earlier run
        self.ticks = 0
        self.age = 0
        self._solved = False
        self._ready = True

    def set_instance_params(self, model=None, plant=None):
        """a fleet: one row of plant parameters per instance, [batch, param_count] each (NumPy or CUDA tensor).  model: what the controller
        believes (every evaluation of the SQP loop and the rollout tail); plant: what the simulated plant step F(s_0, u_0) between two ticks
        uses -- unset, the plant is the controller's model.  None returns that set to the model's shared values.  A plant-model mismatch
        is then studied on the device: nominal controller, randomised plants (examples/fleet_mpc.py)."""
        for v in (model, plant):
            if v is not None and int(np.shape(v)[0]) != self.batch:
                raise ValueError("expected %d rows, one per instance" % self.batch)
        self.ev.set_instance_params(model, plant=False)
        self.ev.set_instance_params(plant, plant=True)

    def set_stage_data(self, d):
        """different worlds: one row of stage data per frame and instance, [batch, horizon, nsd] (NumPy or CUDA tensor) -- what the model's hfun,
        lcost and lterm read as self.sdata (an obstacle's predicted path, a scheduled weight).  Every tick moves the stored set up by one frame
        after the hand-over (tick's d_new enters at the end of the horizon).  None returns to the model's defaults, which do not move."""
        if d is not None and int(np.shape(d)[0]) != self.batch:
            raise ValueError("expected %d instances" % self.batch)
        self.ev.set_stage_data(d)
        self._has_data = d is not None

    @property
    def x(self):
        """the trajectory the next tick starts from [B, N f] (device)"""
        return self.sol.x

    def _arr(self, a, w):
        return None if a is None else self.sol._dev(a, w)

    def tick(self, measured=None, disturbance=None, r_new=None, d_new=None):
        """solve at the pinned first frame, then hand over.  measured [B, nx]: the plant's state after this tick (a real plant); without it
        the model's own map is applied on the device, plus `disturbance` [B, nx] when given.  r_new [B, nx]: the reference entering the
        horizon (per_frame_reference models; omitted: the last one repeats).  d_new [B, nsd]: the stage-data row entering the horizon (a stored
        set only; omitted: the last row repeats); the set shifts with shift=False as well, like the references.  Returns device tensors, overwritten by the next tick:
        applied [B, f] (the frame that was applied), status, iters [B] of the tick's last QP, stage_cost [B] (the k = 0 cost term)."""
        import torch
        if d_new is not None and not self.shift_data:
            raise ValueError("d_new with shift_data=False: the stored rows belong to horizon positions and do not move")
        if not self._ready:
            raise RuntimeError("call reset(frame0, reference) first")
        sol, ev = self.sol, self.ev
        if r_new is not None and not ev.per_frame_reference:
            raise ValueError("r_new belongs to per_frame_reference models")
        if d_new is not None and not self._has_data:
            raise ValueError("d_new needs a stored set of stage data (set_stage_data)")
        sol.getOptimalSolution({"p": self.p, "lbx": self.lbx, "ubx": self.ubx, "lbg": self.lbg, "ubg": self.ubg}, to_host=False)
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        if self.feedback is not None:      # the gains around this tick's plan, from the system the solve just used; the clamp reads the new iterate
            ev.riccati(sol.ls, x=sol.x, lbx=self.lbx, ubx=self.ubx, K=self.K, V=False, failed=self.gain_failed, stream=stream, **self.feedback)
            self.plan.copy_(sol.x)
        self.age = 0
        self._solved = True
        pf = ev.per_frame_reference
        moved = self.shift and sol.warm_start_admm
        ev.advance(sol.x, self._x2, self.lbx, self.ubx, status=sol.status, s_meas=self._arr(measured, ev.nx), w=self._arr(disturbance, ev.nx),
                   tail=self.tail, p=None if pf else self.p, p_in=self.p if pf else None, p_out=self._p2, r_new=self._arr(r_new, ev.nx) if pf else None,
                   dw_in=sol.dw if moved else None, dw_out=self._dw2 if moved else None, y_in=sol.y if moved else None,
                   y_out=self._y2 if moved else None, applied=self.applied, stage_cost=self.stage_cost, stream=stream)
        if self._has_data and self.shift_data:       # after advance, whose stage_cost log and plant step still took d_0
            ev.shift_stage_data(self._arr(d_new, ev.nsd), stream=stream)
        if pf:
            self.p, self._p2 = self._p2, self.p
        if self.shift and sol.direct_active is not None:      # the held set moves with the plan: frame k + 1's entries to frame k, the last frame repeats
            self._act2[:, :-1].copy_(sol.act[:, 1:]); self._act2[:, -1].copy_(sol.act[:, -1])
            sol.act, self._act2 = self._act2, sol.act
            sol._dq["act"] = sol.act
        if self.shift:
            sol.x, self._x2 = self._x2, sol.x
            if moved:
                sol.dw, self._dw2 = self._dw2, sol.dw
                sol.y, self._y2 = self._y2, sol.y
                sol._start_clean = True          # advance left zeros where the QP failed: no NaN to wash out of the start
        self.ticks += 1
        return {"applied": self.applied, "status": sol.status, "iters": sol.iters, "stage_cost": self.stage_cost}

    def hold(self, measured=None, disturbance=None, r_new=None, d_new=None):
        """a plant step without a solve (feedback= only): the hand-over of tick with every instance taking its plan's next input, then one
        mpcqp_stage_feedback launch that corrects the new first frame's input to u = clip(u_1 + K_k (s - s_1)), k = age + 1, age the holds since the
        last tick: s the new first-frame state, (s_1, u_1) frame 1 of the trajectory before the shift, the clip frame 1's input box in lbx / ubx.
        The corrected input is pinned in lbx / ubx like the rest of the first frame.  An instance whose sweep failed at a frame >= k has a zero
        gain there and keeps the plan's input.  Arguments and the data shift as in tick.  Returns device tensors applied [B, f], du [B, nu] (the
        correction), stage_cost [B]."""
        import torch
        if self.feedback is None:
            raise ValueError("hold needs the feedback gains: create the controller with feedback=True")
        if not self.shift:
            raise ValueError("hold with shift=False: the plan does not move between ticks, so there is no next frame to track")
        if not self._ready or not self._solved:
            raise RuntimeError("hold follows a tick: call reset(frame0, reference) and tick() first")
        sol, ev = self.sol, self.ev
        k = self.age + 1
        if k > ev.horizon - 2:
            raise ValueError("hold: the plan is exhausted (%d holds since the last tick on a horizon of %d frames): tick() again" % (self.age, ev.horizon))
        if d_new is not None and not self.shift_data:
            raise ValueError("d_new with shift_data=False: the stored rows belong to horizon positions and do not move")
        if r_new is not None and not ev.per_frame_reference:
            raise ValueError("r_new belongs to per_frame_reference models")
        if d_new is not None and not self._has_data:
            raise ValueError("d_new needs a stored set of stage data (set_stage_data)")
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        pf = ev.per_frame_reference
        moved = sol.warm_start_admm
        nx, f = ev.nx, ev.nx + ev.nu
        ev.advance(sol.x, self._x2, self.lbx, self.ubx, status=None, s_meas=self._arr(measured, ev.nx), w=self._arr(disturbance, ev.nx),
                   tail=self.tail, p=None if pf else self.p, p_in=self.p if pf else None, p_out=self._p2, r_new=self._arr(r_new, ev.nx) if pf else None,
                   dw_in=sol.dw if moved else None, dw_out=self._dw2 if moved else None, y_in=sol.y if moved else None,
                   y_out=self._y2 if moved else None, applied=self.applied, stage_cost=self.stage_cost, stream=stream)
        # advance wrote the first f entries of lbx / ubx only: frame 1 still carries the frame box
        ev.feedback(self.K, k, self._x2[:, :nx], sol.x[:, f:f + nx], sol.x[:, f + nx:2 * f], self._x2, lo=self.lbx[:, f + nx:2 * f],
                    hi=self.ubx[:, f + nx:2 * f], lbx=self.lbx, ubx=self.ubx, du=self.du, stream=stream)
        if self._has_data and self.shift_data:
            ev.shift_stage_data(self._arr(d_new, ev.nsd), stream=stream)
        if pf:
            self.p, self._p2 = self._p2, self.p
        sol.x, self._x2 = self._x2, sol.x
        if moved:
            sol.dw, self._dw2 = self._dw2, sol.dw
            sol.y, self._y2 = self._y2, sol.y
            sol._start_clean = True
        self.age += 1
        return {"applied": self.applied, "du": self.du, "stage_cost": self.stage_cost}

    def close(self):
        self.sol.close()
