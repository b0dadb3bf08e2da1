classdef HipSim < handle
	%HipSim  B independent rollouts of one redmax.Scene on one or several MI355X (libredmax_hip.so through redmax_hip_mex).
	%
	%   sim = redmax.HipSim(scene, batch, devices)  scene: an initialised redmax.Scene (or a desc struct); devices: a device
	%                                               index or a VECTOR of them, e.g. 0:7 - the batch is split into one contiguous
	%                                               shard per entry, every array below stays the whole batch
	%   sim.setState(q, qdot)                       nr x batch, the DOF order of Joint.getQ
	%   [T,V,stats,Q,Qdot] = sim.step(itype, h, nsteps, opts)   itype 1: BDF1, 2: SDIRK2 + BDF2; all devices step concurrently
	%   sim.stepAsync(itype, h, nsteps, opts, record);  ...  [T,V,stats,Q,Qdot] = sim.sync();   the same, MATLAB free in between
	%   [q, qdot] = sim.getState()
	%   delete(sim)
	%
	% Replaces the interpreter-side simLoop / newton / evalBDF1 / computeValues of matlab-diff/driverRedMaxBDF1.m:57-243
	% (and driverRedMaxBDF2.m) for a whole batch of trajectories; the Scene/Joint/Body classes are the reference's.

	properties (SetAccess = private)
		h      % uint64 handle of the gateway
		nr     % reduced DOFs
		nm     % maximal DOFs
		nsph   % spherical joints (Euler charts live on the device, see getCharts)
		batch  % trajectories
		idxR   % 0-based reduced index of every listed joint's first DOF (-1: fixed)
		devices      % device of every shard
		shardFirst   % 0-based index of every shard's first trajectory
		shardCount   % trajectories per shard
	end

	methods
		function this = HipSim(scene, batch, devices)
			if nargin < 2, batch = 1; end
			if nargin < 3, devices = 0; end
			if isstruct(scene)
				desc = scene;
			else
				desc = redmax.flattenScene(scene);
			end
			this.h = redmax_hip_mex('create', desc, batch, double(devices(:)'));
			info = redmax_hip_mex('info', this.h);
			this.nr = info.nr; this.nm = info.nm; this.nsph = info.nsph; this.batch = info.batch; this.idxR = info.idxR;
			this.devices = info.devices; this.shardFirst = info.shard_first; this.shardCount = info.shard_count;
		end

		function delete(this)
			if ~isempty(this.h)
				redmax_hip_mex('destroy', this.h);
				this.h = [];
			end
		end

		function setState(this, q, qdot)
			% Joint.setQ for the batch; a single column is replicated over the batch
			if size(q,2) == 1 && this.batch > 1
				q = repmat(q, 1, this.batch); qdot = repmat(qdot, 1, this.batch);
			end
			redmax_hip_mex('set', this.h, q, qdot);
		end

		function [q, qdot] = getState(this)
			[q, qdot] = redmax_hip_mex('get', this.h);
		end

		function varargout = step(this, itype, hstep, nsteps, opts)
			if nargin < 5, opts = struct(); end
			[varargout{1:max(nargout,1)}] = redmax_hip_mex('step', this.h, itype, hstep, nsteps, opts);
		end

		function stepAsync(this, itype, hstep, nsteps, opts, record)
			% launch simLoop on every device and return; record: 1 = T, V (default), +2 = Q, Qdot, +4 = charts
			if nargin < 5 || isempty(opts), opts = struct(); end
			if nargin < 6, record = 1; end
			redmax_hip_mex('step_async', this.h, itype, hstep, nsteps, opts, record);
		end

		function varargout = sync(this)
			% wait for the launches of stepAsync and gather: [T, V, stats, Q, Qdot, C] as step
			[varargout{1:max(nargout,1)}] = redmax_hip_mex('sync', this.h);
		end

		function [wall, kernel, t0, t1] = timing(this)
			% wall clock ms of the last step and, per shard, kernel ms and launch start / end (rmx_group_timing)
			[wall, kernel, t0, t1] = redmax_hip_mex('timing', this.h);
		end

		function t = ticks(this)
			% shader-clock ticks every rollout's wavefront spent in the last step launch (rmx_step_ticks)
			t = redmax_hip_mex('ticks', this.h);
		end

		function [T, V] = euler(this, hstep, nsteps)
			[T, V] = redmax_hip_mex('euler', this.h, hstep, nsteps);
		end

		function varargout = evalResidual(this, q, qA, qB, eta)
			% g (and H when two outputs are requested): evalBDF1 is evalResidual(q1, q0, q0 + h*qdot0, h)
			[varargout{1:max(nargout,1)}] = redmax_hip_mex('eval', this.h, q, qA, qB, eta);
		end

		function varargout = computeValues(this, q, qdot, varargin)
			% [M,f,K,D,dMv] = computeValues(q, qdot [, v]): the full output of the reference's computeValues (driverRedMaxBDF1.m:188-243)
			% at (q, qdot), per rollout; dMv(:,i,b) = dMdq(:,:,i) * v(:,b)
			[varargout{1:max(nargout,1)}] = redmax_hip_mex('values', this.h, q, qdot, varargin{:});
		end

		function [T, V] = energy(this)
			[T, V] = redmax_hip_mex('energy', this.h);
		end

		function [q, qdot, path] = gather(this, root)
			% the final gather of the sharded batch with device-resident destinations (rmx_group_gather: RCCL over the group's devices):
			% every shard's device (root omitted) or shard `root`'s device alone (0-based) ends up with the whole batch; q, qdot (nr x batch):
			% that copy read back; path: 'rccl:allgather' | 'rccl:broadcast' | 'rccl:sendrecv' | 'copy'
			if nargin < 2
				root = -1;
			end
			[q, qdot, path] = redmax_hip_mex('gather', this.h, root);
		end

		function c = getCharts(this)
			c = redmax_hip_mex('getcharts', this.h);
		end

		function setCharts(this, c)
			redmax_hip_mex('setcharts', this.h, int32(c));
		end

		function on = tapePointForces(this, enable)
			% rmx_model_tape_point_forces: enable true (default) - rolloutTape, rolloutFeedback and rolloutFeedbackBox take a model with
			% point forces (ForcePointPoint / ForceSpringDamper / ForceCable) and leave a tape whose H and D carry them, which
			% rolloutVjp, rolloutLinearize, rolloutJvp, rolloutVjpFeedback and rolloutLqr[Box] read unchanged; false restores the
			% refusal.  A model without such forces is not affected.  on: the switch as read back.
			if nargin < 2
				enable = true;
			end
			on = redmax_hip_mex('tape_point_forces', this.h, double(logical(enable))) ~= 0;
		end

		function [P, dPdp, stats] = adjoint(this, hstep, nsteps, task, p, itype)
			% taskObjective of driverRedMaxAdjointBDF1.m (itype 1, default) / driverRedMaxAdjointBDF2.m (itype 2)
			if nargin < 6
				itype = 1;
			end
			[P, dPdp, stats] = redmax_hip_mex('adjoint', this.h, hstep, nsteps, task, p, itype);
		end

		function [P, dPdu, stats] = adjointControls(this, hstep, nsteps, task, u, itype)
			% the adjoint with one torque per joint and step (task.applyStep at every step): u, dPdu are nr x nsteps x B;
			% at step k the joint torque is tau + task.pscale*u(:,k,b).  itype 1 (BDF1, default) / 2 (BDF2).
			% With one output, P = sim.adjointControls(...), only the forward rollout runs.
			if nargin < 6
				itype = 1;
			end
			if nargout < 2
				P = redmax_hip_mex('adjoint_controls', this.h, hstep, nsteps, task, u, itype);
			else
				[P, dPdu, stats] = redmax_hip_mex('adjoint_controls', this.h, hstep, nsteps, task, u, itype);
			end
		end

		function [P, dPdu, stats] = adjointTrack(this, hstep, nsteps, task, u, itype)
			% adjointControls with a tracking objective: task.terms is a struct array with the fields body (1-based),
			% xlocal, step and wpos - point targets on several bodies at several steps -, task.xtarget is 3 x nterms (one
			% target table for the batch) or 3 x nterms x B (one per rollout), task.pscale and task.wreg as before.
			% P(b) = sum_i wpos_i/2 |x_i(step_i) - xtarget(:,i,b)|^2 + wreg/2 sum u(:,:,b).^2 ; u, dPdu: nr x nsteps x B.
			% With one output only the forward rollout runs.
			if nargin < 6
				itype = 1;
			end
			if nargout < 2
				P = redmax_hip_mex('adjoint_track', this.h, hstep, nsteps, task, u, itype);
			else
				[P, dPdu, stats] = redmax_hip_mex('adjoint_track', this.h, hstep, nsteps, task, u, itype);
			end
		end

		function [qtraj, qdtraj, stats] = rolloutTape(this, hstep, nsteps, pscale, u, integrator)
			% a controlled BDF1 (or, integrator 2, BDF2) rollout from the current state that records its trajectory and keeps the tape rolloutVjp
			% reads: u, qtraj, qdtraj are nr x nsteps x B; at step k the joint torque is tau + pscale*u(:,k,b) and
			% qtraj(:,k,b), qdtraj(:,k,b) is the state after it.  There is no objective: it is the caller's.
			% integrator (optional, default 1) 2: the BDF2 rollout, self-started with SDIRK2 from the current state (step 1,
			% whose torque holds for both stages); rolloutVjp then differentiates the start step exactly as well.
			if nargin < 6
				integrator = 1;
			end
			[qtraj, qdtraj, stats] = redmax_hip_mex('rollout_tape', this.h, hstep, nsteps, pscale, u, integrator);
		end

		function [qtraj, qdtraj, uapp, stats] = rolloutFeedback(this, hstep, nsteps, pscale, uff, K, xref, integrator)
			% rolloutTape in closed loop (the forward pass of iLQR, time-varying LQR tracking): the torque of step k is
			%   uapp(:,k,b) = uff(:,k,b) + K(:,:,k) * (x - xref(:,k)),   x = [q; qdot] at the START of step k,
			% formed on the device from the state the rollout has reached - all steps in one launch.  uff: nr x nsteps x B.
			% K: nr x 2nr x nsteps, shared by the batch, or nr x 2nr x nsteps x B, K(i,j,k) = du_i/dx_j; xref: 2nr x nsteps
			% or 2nr x nsteps x B (K and xref alike); [] for either: no feedback / a zero reference.  uapp: the applied torques.
			% The tape it leaves is the open-loop tape under uapp: rolloutVjp, rolloutLinearize and rolloutJvp differentiate
			% that open-loop rollout; rolloutVjpFeedback differentiates the closed loop (dL/dK, dL/dxref, dL/duff).
			if nargin < 6
				K = [];
			end
			if nargin < 7
				xref = [];
			end
			if nargin < 8
				integrator = 1;
			end
			[qtraj, qdtraj, uapp, stats] = redmax_hip_mex('rollout_feedback', this.h, hstep, nsteps, pscale, uff, K, xref, integrator);
		end

		function [du, dq0, dqd0] = rolloutVjp(this, nsteps, gq, gqd)
			% the gradient of any loss L on the trajectory of the last rolloutTape: gq, gqd (nr x nsteps x B) are dL/dq and
			% dL/dqdot of every step; du (nr x nsteps x B), dq0, dqd0 (nr x B) are dL/du, dL/dq0, dL/dqdot0.  May be
			% repeated with other cotangents; an adjoint* call or another rolloutTape ends the tape.
			[du, dq0, dqd0] = redmax_hip_mex('rollout_vjp', this.h, nsteps, gq, gqd);
		end

		function [duff, dK, dxref, dq0, dqd0] = rolloutVjpFeedback(this, nsteps, gq, gqd, K, xref, gu)
			% the closed-loop adjoint of the last rolloutFeedback: gq, gqd as rolloutVjp, gu (nr x nsteps x B, or []: zero) the
			% cotangent of the applied torques uapp; K, xref: the tables of the forward call ([]: no gains / a zero reference).
			% duff (nr x nsteps x B), dK (nr x 2nr x nsteps x B), dxref (2nr x nsteps x B), dq0, dqd0 (nr x B): ALWAYS one slice
			% per rollout - for tables the batch shares, sum over B.  Outputs that are not asked for are not formed; without
			% gains dK and dxref are [].  The tape and the state stay as they are.
			if nargin < 7
				gu = [];
			end
			[duff, dK, dxref, dq0, dqd0] = redmax_hip_mex('rollout_vjp_feedback', this.h, nsteps, gq, gqd, K, xref, gu);
		end

		function [du, dq0, dqd0, grads] = rolloutVjpParams(this, nsteps, gq, gqd)
			% rolloutVjp (the same du, dq0, dqd0) and the gradient of the loss with respect to the model's parameters, one column
			% per rollout: grads.stiffness, grads.damping, grads.qrest (nr x B, reduced DOF order), grads.inertia (6 x njoints x B,
			% the layout of desc.I_i) and grads.grav (3 x B).  The gradient of a parameter the rollouts share is the sum over B;
			% of a stiffness or damping set per joint the sum over that joint's DOFs.  The tape and the state stay as they are.
			[du, dq0, dqd0, dk, dd, dr, dI, dg] = redmax_hip_mex('rollout_vjp_params', this.h, nsteps, gq, gqd);
			grads = struct('stiffness', dk, 'damping', dd, 'qrest', dr, 'inertia', dI, 'grav', dg);
		end

		function [du, dq0, dqd0, fgrads, grads] = rolloutVjpForces(this, nsteps, gq, gqd, nforces)
			% rolloutVjpParams for a tape that carries point forces (tapePointForces): rolloutVjp (the same du, dq0, dqd0), the
			% gradient with respect to the constants of the nforces rows of the force table, one column per rollout -
			% fgrads.stiffness, fgrads.damping, fgrads.L (nforces x B; a point-point force has no rest length, its L entry is 0) -
			% and, where asked for, grads as rolloutVjpParams returns it.  The tape and the state stay as they are.
			if nargout > 4
				[du, dq0, dqd0, dks, dkd, dL, dk, dd, dr, dI, dg] = redmax_hip_mex('rollout_vjp_forces', this.h, nsteps, gq, gqd, nforces);
				grads = struct('stiffness', dk, 'damping', dd, 'qrest', dr, 'inertia', dI, 'grav', dg);
			else
				[du, dq0, dqd0, dks, dkd, dL] = redmax_hip_mex('rollout_vjp_forces', this.h, nsteps, gq, gqd, nforces);
			end
			fgrads = struct('stiffness', dks, 'damping', dkd, 'L', dL);
		end

		function [XA, XB, XU] = rolloutLinearize(this, nsteps)
			% the linearisation of the last rolloutTape: the sensitivities XA = dx/dqA, XB = dx/dqB, XU = dx/du of every taped
			% solve x(qA, qB, u), each nr x nr x nslots x B with (i,j,s,b) = dx_i/d(.)_j of slot s; nslots = nsteps, or
			% nsteps + 1 after a BDF2 rolloutTape (the last slot is the SDIRK2a solve).  Under BDF1, with h the step size,
			%   A_k = [XA+XB, h*XB; (XA+XB-I)/h, XB]   B_k = [XU; XU/h]   (state order (q, qdot); slices (:,:,k,b))
			% Outputs that are not asked for are not computed.  The tape and the state stay as they are.
			XA = []; XB = []; XU = [];
			if nargout <= 1
				XA = redmax_hip_mex('rollout_linearize', this.h, nsteps);
			elseif nargout == 2
				[XA, XB] = redmax_hip_mex('rollout_linearize', this.h, nsteps);
			else
				[XA, XB, XU] = redmax_hip_mex('rollout_linearize', this.h, nsteps);
			end
		end

		function [tq, tqd] = rolloutJvp(this, nsteps, tu, tq0, tqd0)
			% forward-mode tangents of the last rolloutTape: for tangents of the controls tu (nr x nsteps x T x B) and of the initial
			% state tq0, tqd0 (nr x T x B), T directions per rollout in one sweep over the tape, tq and tqd (nr x nsteps x T x B)
			% are the tangents of the state after every step.  [] for any of the three means zero (not all).  With du, dq0, dqd0
			% of rolloutVjp for cotangents gq, gqd:  gq(:)'*tq(:) + gqd(:)'*tqd(:) == du(:)'*tu(:) + dq0(:)'*tq0(:) + dqd0(:)'*tqd0(:).
			% The tape and the state stay as they are.
			if nargin < 4
				tq0 = [];
			end
			if nargin < 5
				tqd0 = [];
			end
			[tq, tqd] = redmax_hip_mex('rollout_jvp', this.h, nsteps, tu, tq0, tqd0);
		end

		function [tq, tqd] = rolloutJvpParams(this, nsteps, tp, tu, tq0, tqd0)
			% forward-mode tangents of the last rolloutTape with respect to the model's parameters: rolloutJvp with the parameter
			% term on the right of every taped solve.  tp: a struct with any of the fields stiffness, damping, qrest (nr x T x B,
			% per reduced DOF), inertia (6 x njoints x T x B, the layout of I_i: a mass tangent is the same number in entries
			% 4..6) and grav (3 x T x B), at least one; a missing or empty field means zero.  tu, tq0, tqd0 as rolloutJvp
			% (optional).  tq, tqd (nr x nsteps x T x B).  It is the transpose of rolloutVjpParams: with its outputs for cotangents
			% gq, gqd, gq(:)'*tq(:) + gqd(:)'*tqd(:) equals rolloutJvp's right-hand side plus dk(:)'*tp.stiffness(:) + ... over
			% the five groups.  Columns of the Jacobian for Gauss-Newton / Levenberg-Marquardt identification: one unit direction
			% per parameter entry, all in one call.  The tape and the state stay as they are.
			if nargin < 4
				tu = [];
			end
			if nargin < 5
				tq0 = [];
			end
			if nargin < 6
				tqd0 = [];
			end
			names = {'stiffness', 'damping', 'qrest', 'inertia', 'grav'};
			args = cell(1, 5);
			for i = 1:5
				if isfield(tp, names{i})
					args{i} = tp.(names{i});
				else
					args{i} = [];
				end
			end
			[tq, tqd] = redmax_hip_mex('rollout_jvp_params', this.h, nsteps, args{:}, tu, tq0, tqd0);
		end

		function [kff, K, expected, notpd] = rolloutLqr(this, nsteps, lx, lu, Q, R, mu)
			% the Riccati sweep of iLQR on the BDF1 tape of the last rolloutTape / rolloutFeedback, in one launch: for the cost's
			% gradients at the nominal lx (2nr x nsteps x B), lu (nr x nsteps x B) and its Hessians Q (2nr x 2nr x nsteps, shared,
			% or 2nr x 2nr x nsteps x B) and R (nr x nr), both symmetric, the feed-forward kff (nr x nsteps x B) and the gains
			% K (nr x 2nr x nsteps x B, K(i,j,k,b) = du_i/dx_j) that rolloutFeedback takes as they are: one iLQR trial is
			% rolloutFeedback(hstep, nsteps, pscale, ubar + alpha*kff, K, xbar).  mu >= 0 (default 0) regularises Quu.  expected
			% (1 x B): the decrease of the quadratic model under the full step; notpd (1 x B): 1 where Quu + mu*I was not
			% positive definite - that rollout's gains are zero.  The tape and the state stay as they are.
			if nargin < 7
				mu = 0;
			end
			[kff, K, expected, notpd] = redmax_hip_mex('rollout_lqr', this.h, nsteps, lx, lu, Q, R, mu);
		end

		function [qtraj, qdtraj, uapp, stats] = rolloutFeedbackBox(this, hstep, nsteps, pscale, uff, K, xref, ulo, uhi, integrator)
			% rolloutFeedback with torque limits: uapp = min(max(uff + K*(x - xref), ulo), uhi) per DOF, clamped on the device
			% behind the feedback sum (with K = [] too: actuator saturation of an open-loop torque).  ulo, uhi: nr elements, or
			% []: that side is unbounded.  Everything else is rolloutFeedback's; rolloutVjpFeedback does not know about the clamp.
			if nargin < 10
				integrator = 1;
			end
			[qtraj, qdtraj, uapp, stats] = redmax_hip_mex('rollout_feedback_box', this.h, hstep, nsteps, pscale, uff, K, xref, ulo, uhi, integrator);
		end

		function [kff, K, expected, status, clamped] = rolloutLqrBox(this, nsteps, lx, lu, Q, R, ubar, ulo, uhi, mu, maxIter)
			% rolloutLqr under the torque limits ulo <= u <= uhi (control-limited DDP): at every step the box QP over
			% ulo - ubar_k <= k <= uhi - ubar_k in the place of the solve; ubar (nr x nsteps x B) are the nominal applied torques,
			% the uapp of the rolloutFeedbackBox call that left the tape.  A torque on a bound has kff = bound - ubar exactly and
			% a zero row of K.  status (1 x B): 0, 1 (a pivot not > 0), 2 (a QP did not terminate within maxIter, default 64) - the
			% gains of such a rollout are zero; clamped (nsteps x B): bit i-1 set where DOF i of the step ended on a bound.
			if nargin < 10
				mu = 0;
			end
			if nargin < 11
				maxIter = 0;
			end
			[kff, K, expected, status, clamped] = redmax_hip_mex('rollout_lqr_box', this.h, nsteps, lx, lu, Q, R, ubar, ulo, uhi, mu, maxIter);
		end

		function [x, gq] = rolloutPoints(this, nsteps, q, terms, gx)
			% World positions of body points along a state record q (nr x nsteps x batch; any record, typically a qtraj):
			% x is 3 x nterms x batch.  terms: struct array with the fields body (1-based listing index), xlocal, step - the
			% point of term t is read at the posture q(:, step_t, b).  With gx (3 x nterms x batch), gq (nr x nsteps x batch) is the
			% pull-back sum_t Jp_t' * gx_t over the terms of each step, Jp_t the Jacobian of the point AT THAT STATE.  Needs no
			% tape and leaves the tape alone.
			if nargin < 5
				x = redmax_hip_mex('rollout_points', this.h, nsteps, q, terms);
				gq = [];
			else
				[x, gq] = redmax_hip_mex('rollout_points', this.h, nsteps, q, terms, gx);
			end
		end

		function [Jk, lx, Q] = rolloutCost(this, nsteps, q, qdot, Qin, xgoal, terms, xtarget)
			% The cost of a state record and its second-order model for rolloutLqr: the joint-space quadratic Qin (2nr x 2nr x
			% nsteps [x batch], symmetric) about xgoal (2nr x nsteps [x batch]) plus point targets - terms (struct array body,
			% xlocal, step, wpos >= 0) and xtarget (3 x nterms [x batch]).  [] for Qin, xgoal: zero; [] for terms: no targets.
			% Jk (nsteps x batch) = 1/2 dx'*Qin*dx + sum_t w_t/2 |p_t - xtarget_t|^2; lx (2nr x nsteps x batch) its exact gradient;
			% Q (2nr x 2nr x nsteps x batch) = Qin + sum_t w_t Jp_t'*Jp_t in the q block - the Gauss-Newton model (the curvature of
			% the points is dropped), the per-rollout table rolloutLqr takes.  Needs no tape and leaves the tape alone.
			if nargin < 8
				xtarget = [];
			end
			if nargin < 7
				terms = [];
			end
			[Jk, lx, Q] = redmax_hip_mex('rollout_cost', this.h, nsteps, q, qdot, Qin, xgoal, terms, xtarget);
		end

		function [x, v, R, gq, gqd] = rolloutFrames(this, nsteps, q, qdot, terms, gx, gv, gR)
			% Position x and point velocity v (3 x nterms x batch) and orientation R (3 x 3 x nterms x batch) of body frames
			% along a state record q, qdot (nr x nsteps x batch).  terms: struct array with the fields body (1-based listing
			% index), xlocal, step - the frame of term t is read at the state of column step_t; weights are not read.  With
			% cotangents gx, gv (3 x nterms x batch) and gR (3 x 3 x nterms x batch), [] for zero, gq and gqd (nr x nsteps x
			% batch) are the pull-backs sum_t Jp'*gx + G'*gv + Jw'*a(gR*R') and sum_t Jp'*gv, with Jp = dp/dq = dv/dqdot,
			% G = dv/dq and Jw the angular Jacobian AT THAT STATE.  Needs no tape and leaves the tape alone.
			if nargin < 6
				[x, v, R] = redmax_hip_mex('rollout_frames', this.h, nsteps, q, qdot, terms);
				gq = [];
				gqd = [];
				return
			end
			if nargin < 7
				gv = [];
			end
			if nargin < 8
				gR = [];
			end
			[x, v, R, gq, gqd] = redmax_hip_mex('rollout_frames', this.h, nsteps, q, qdot, terms, gx, gv, gR);
		end

		function [Jk, lx, Q] = rolloutCostFrames(this, nsteps, q, qdot, Qin, xgoal, terms, xtarget, vtarget, Rtarget)
			% rolloutCost with frame terms: terms is a struct array body, xlocal, step and the weights wpos, wvel, wrot >= 0 (a
			% missing one is 0); xtarget, vtarget (3 x nterms [x batch]) and Rtarget (3 x 3 x nterms [x batch]) are the targets
			% of the point's position, its velocity and the body's orientation, [] for a table no term weighs.  Per term
			% wpos/2 |p - xtarget|^2 + wvel/2 |v - vtarget|^2 + wrot/4 |R - Rtarget|_F^2 (the last is wrot (1 - cos theta); its
			% gradient vanishes at theta = pi).  lx is the exact gradient in (q, qdot); Q is the Gauss-Newton table with the
			% velocity terms' q, qdot cross blocks, symmetric bit for bit.  Needs no tape and leaves the tape alone.
			if nargin < 10
				Rtarget = [];
			end
			if nargin < 9
				vtarget = [];
			end
			if nargin < 8
				xtarget = [];
			end
			[Jk, lx, Q] = redmax_hip_mex('rollout_cost_frames', this.h, nsteps, q, qdot, Qin, xgoal, terms, xtarget, vtarget, Rtarget);
		end

		function [qtraj, qdtraj, uapp, J, alpha, stats] = rolloutSearch(this, hstep, nsteps, pscale, ubar, kff, K, xref, alphas, Jbar, cost, ulo, uhi)
			% The backtracking line search of iLQR in ONE launch (rmx_rollout_search, BDF1): from the current state every rollout
			% runs the closed loop of rolloutFeedback (K, xref as there) under uff = ubar + a*kff for a in alphas, in order, and
			% keeps the first pass without a failed solve whose cost is below its Jbar; a rollout no alpha helps - and every
			% rollout with alphas = [], where kff and Jbar may be [] - runs the nominal pass uff = ubar.  cost is a struct with the
			% fields Q, xgoal, terms, xtarget, vtarget, Rtarget (as rolloutCostFrames takes them) and R (nr x nr), each optional:
			% J = sum_k 1/2 dx'Q dx + 1/2 u'R u + the terms, on the states each pass produces and its APPLIED torques.  ulo, uhi
			% (nr, [] for no bound on that side): the torque limits of rolloutFeedbackBox.  J, alpha: 1 x batch (alpha 0: none
			% accepted); qtraj, qdtraj, uapp, stats and the tape belong to the pass each rollout kept.  One iLQR iteration is
			% rolloutCost[Frames], rolloutLqr[Box], rolloutSearch.
			if nargin < 13
				[qtraj, qdtraj, uapp, J, alpha, stats] = redmax_hip_mex('rollout_search', this.h, hstep, nsteps, pscale, ubar, kff, K, xref, alphas, Jbar, cost);
			else
				[qtraj, qdtraj, uapp, J, alpha, stats] = redmax_hip_mex('rollout_search', this.h, hstep, nsteps, pscale, ubar, kff, K, xref, alphas, Jbar, cost, ulo, uhi);
			end
		end
	end
end
