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
    def __init__(self, model, options=None, batch=1, tail="rollout", shift=True, device=-1, codegen=None, shift_data=True):
        """model: a models.StageOCP (zoo, generated or per_frame_reference).  options: those of DeviceSQPOptimizationSolver, passed through
        (warm_start_admm, carry_rho, constant_matrices, keep_scaling, presolve_fixed_rows, ...); max_iter defaults to 1 SQP iteration per
        tick and alpha to 1 (real-time iteration), skip_failed_steps to True (an infeasible QP keeps its iterate and holds the input).
        shift_data=False: a tick does not shift the stored stage data -- rows that belong to horizon positions, not to world time (the step
        lengths of a non-uniform time grid, models.StageOCP.transition_data); tick's d_new is then a ValueError."""
        import torch
        if tail not in ("repeat", "rollout"):
            raise ValueError("tail must be 'repeat' or 'rollout'")
        opts = dict(options or {})
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
        self.ticks = 0
        self._ready = False
        self._has_data = False
        self.rollout_diverged = None; self.rollout_box_viol = None

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
        self.ticks = 0
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
        if self.shift:
            sol.x, self._x2 = self._x2, sol.x
            if moved:
                sol.dw, self._dw2 = self._dw2, sol.dw
                sol.y, self._y2 = self._y2, sol.y
                sol._start_clean = True          # advance left zeros where the QP failed: no NaN to wash out of the start
        self.ticks += 1
        return {"applied": self.applied, "status": sol.status, "iters": sol.iters, "stage_cost": self.stage_cost}

    def close(self):
        self.sol.close()
