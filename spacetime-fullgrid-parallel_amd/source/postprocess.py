"""What both solve drivers (heateq.py, heateq_mpi.py) offer on a solution once it is there:
sampling, its adjoint, the history maps, the time curves, the solidification maps, the
isotherms, the error norms, the prolongation of a coarser level's vector and the restriction
of a functional to a coarser level -- the eleven public methods, once, with the plans they build on first use.

A driver inherits ``PostProcessing``, calls ``_init_postprocessing`` from its constructor and
supplies what truly differs as two hooks: how `u` becomes a trial-space device vector
(``_trial_vector``) and what ``sample_along_adjoint`` builds on (``_adjoint_target``).
"""


class PostProcessing:
    """The post-processing methods of HeatEquation and HeatEquationMPI.  `u` is a trial-space
    vector: a KronVectorMPI in heateq_mpi.py; heateq.py takes a flat NumPy vector or a device
    vector (source.linop.device_vector)."""

    def _init_postprocessing(self, mesh_space, mesh_time, data):
        """The plans are built by the first call that needs them, from these meshes; `data`
        is the problem's (its exact solution, if it has one, is what error_norms() compares
        with)."""
        self._sample_meshes = (mesh_space, mesh_time)
        self._exact = (data.get('exact'), data.get('exact_grad'))
        self.sample_plan = self.error_plan = self.curves_plan = self.solid_plan = None
        self.transfer_plans = {}  # per coarse discretisation, built by the first prolong_from() or restrict_to() of it

    # ---- what a driver supplies -----------------------------------------------------------------
    def _trial_vector(self, u, who):
        """`u` as a device vector of the trial space, or AssertionError '`who` takes vectors of
        the trial space'."""
        raise NotImplementedError

    def _adjoint_target(self, out):
        """(the distribution a vector of ``sample_along_adjoint`` is built on, `out` as a device
        vector or None)."""
        raise NotImplementedError

    # ---- the plans, built on first use ----------------------------------------------------------
    def _lazy_plan(self, name, Plan):
        """The plan self.<name>, a Plan(mesh_space, mesh_time) made by the first call."""
        this_plan = getattr(self, name)
        if this_plan is None:
            this_plan = Plan(*self._sample_meshes)
            setattr(self, name, this_plan)
        return this_plan

    def _sample_plan(self):
        from .sampling import SamplePlan
        return self._lazy_plan('sample_plan', SamplePlan)

    def _sample_plan_for(self, u):
        """The sampling plan, once `u` has passed for a vector of the trial space."""
        self._trial_vector(u, 'sampling')
        return self._sample_plan()

    # ---- the eleven methods ---------------------------------------------------------------------
    def sample(self, u, times, points, field='u'):
        """u_h(t_k, x_p) of a trial-space vector `u` (KronVectorMPI: a solution, an iterate)
        at `times` (n_k,) in [0, T] and `points` (n_p, d) -- NumPy array, device tensor, or
        what ``sample_plan.locate`` returned -- as an (n_k, n_p) device tensor, NaN at
        points outside the mesh.  COLLECTIVE: every rank evaluates the terms of the time
        nodes it owns (source/sampling.py, csrc/sample.hip) and the block is all-reduced
        with the communicator of the vectors; every term has one non-zero contributor, so
        the block does not depend on the number of ranks, bit for bit, and every rank
        returns all of it.  The plan (mesh and point-location grid on the device) is built
        by the first call; a run that never samples builds nothing.  Test-space vectors
        (discontinuous in time) are out of scope; paired lists (t_p, x_p) are served by
        ``sample_along``.  field='dt': the block of the time derivative (the right-hand one at
        an interior node, the left-hand one at T); field='grad': the blocks of the gradient,
        shape (d, n_k, n_p); both collective and rank-independent in the same way.  The serial
        driver also takes `u` as a flat NumPy vector or a device vector and returns the same
        device tensors."""
        from .sampling import sample_collective
        u = self._trial_vector(u, 'sampling')
        return sample_collective(self._sample_plan(), u, times, points, field=field)

    def sample_along(self, u, times, points, fields=('u',)):
        """u_h, its time derivative and its gradient of a trial-space vector `u` along a
        trajectory: at the PAIRS (times[p], points[p]), `times` (n_p,) and `points` (n_p, d)
        NumPy arrays or device tensors.  Returns a dict of device tensors: 'u' (n_p,),
        'dt' (n_p,), 'grad' (d, n_p) -- those named in `fields` -- and 'inside' (n_p,) bool;
        NaN where a point is outside the mesh or a time is NaN or outside [0, T] (checked on
        the device).  The work is 2 (d + 1) slab entries per point, never the (n_p, n_p)
        block.  COLLECTIVE and independent of the number of ranks, bit for bit, as
        ``sample``; the plan is built by the first call of either.  The serial driver also takes
        `u` as a flat NumPy vector or a device vector and returns the same dict."""
        from .sampling import sample_pairs_collective
        u = self._trial_vector(u, 'sampling')
        return sample_pairs_collective(self._sample_plan(), u, times, points, fields)

    def sample_along_adjoint(self, weights, times, points, field='u', out=None, accumulate=False):
        """The adjoint E^T of ``sample_along``: numbers given at the PAIRS (times[p], points[p])
        as a functional on the trial space -- v -> sum_p weights[p] v_h(t_p, x_p) for
        field='u', the same with d/dt v_h for 'dt', sum_p weights[:, p] . grad v_h(t_p, x_p)
        for 'grad' (`weights` (n_p,), for 'grad' (d, n_p); NumPy arrays or device tensors;
        `points` also what ``sample_plan.locate`` returned).  Returns (vec, used): a
        KronVectorMPI of the trial space -- `out` if given, overwritten, or added to with
        accumulate=True -- and a device bool tensor (n_p,), False where the point is outside
        the mesh or the time is NaN or outside [0, T] (checked on the device): such a pair
        contributes nothing.  With r = sample_along(u) - data, ``solve(rhs=vec)`` is the
        gradient of the misfit 1/2 |r|^2 with respect to the right-hand side.  Every rank
        passes ALL pairs and builds the columns it owns: no communication, and -- every entry
        being a sum of one fixed order, not an atomic scatter -- independent of the number of
        ranks, bit for bit, as ``sample_along``; the plan is built by the first call of any of
        the sampling methods.  The serial driver returns a DEVICE vector
        (source.linop.host_vector copies it out; ``solve(rhs=vec)`` takes it as it is) and also
        takes `out` as a flat NumPy vector, which is copied to the device, not changed."""
        from .sampling import FIELDS
        if field not in FIELDS:  # before a plan is built for it
            raise ValueError('field must be one of %s, not %r' % (FIELDS, field))
        distribution, out = self._adjoint_target(out)
        plan = self._sample_plan()
        return plan.adjoint_pairs(distribution, weights, times, plan.locate(points), field=field, out=out,
                                  accumulate=accumulate)

    def history_maps(self, u, threshold=None, points=None, fields=None):
        """The thermal history of a trial-space vector `u` (KronVectorMPI) over [0, T], from one
        scan along time on the device (source/history.py, csrc/history.hip): a dict of device
        tensors 'peak' and 't_peak' (the largest nodal value and the earliest node that has
        it), 'dose' (the integral over time, the trapezoid sum of the piecewise linear
        function), 'max_rate' and 'min_rate' (the largest and smallest d/dt u_h), and with a
        `threshold` 'time_above' (how long u_h > threshold), 't_first' and 't_last' (the first
        time it gets above and the last time it is above; NaN if never).  threshold=None scans
        with +inf and leaves those three out.  `fields`: a subset of the names to return.
        Without `points`: (M,) tensors in free-dof order.  With `points` (n_p, d) -- NumPy
        array, device tensor or what ``sample_plan.locate`` returned --: (n_p,) tensors of u_h
        there (through ``sample`` at the nodes, in column chunks of at most 256 MB) plus
        'inside'; NaN in every field at points outside the mesh.  COLLECTIVE and independent of
        the number of ranks, bit for bit: the scan's state travels down the ranks in time order
        (size - 1 transfers of 72 M bytes, serial by design).  A wrong shape, an unknown field
        or a NaN threshold raises ValueError before anything touches the GPU.  Test-space
        vectors are refused.  Out of scope: time windows other than [0, T], several thresholds
        in one call, per-row thresholds.  The serial driver also takes `u` as a flat NumPy
        vector or a device vector and returns the same dict."""
        from .history import check_arguments, history_maps
        check_arguments(threshold, points, self._sample_meshes[0].points.shape[1], fields)  # before an upload or a plan
        u = self._trial_vector(u, 'history_maps()')
        if points is not None:
            self._sample_plan()
        return history_maps(self, u, threshold, points, fields)

    def time_curves(self, u, threshold=None):
        """What a trial-space vector `u` (KronVectorMPI) does over SPACE at every time node
        t_k, k = 0 .. N - 1, from one pass over the cells on the device
        (source/time_curves.py, csrc/curves.hip): a dict of device tensors with one entry per
        node: 'heat' (the integral of u_h over the domain), 'l2_sq' and 'h1_sq' (the integrals
        of u_h^2 and |grad u_h|^2), 'outflow' (minus the integral of the normal derivative over
        the boundary: the heat leaving), 'peak' and 'peak_row' (the largest nodal value over
        the free dofs and the lowest slab row that has it, int64) and 'peak_point' ((N, d), the
        coordinates of that row's vertex); and with a `threshold` the zone {u_h > threshold},
        exact for the P1 function: 'measure_above', 'moment_above' ((N, d), the integral of x
        over the zone), 'centroid_above' ((N, d), NaN where the measure is 0), 'box_lo' and
        'box_hi' ((N, d), NaN where the zone is empty).  A vertex AT the threshold is not above,
        the rule of ``history_maps``; threshold=None leaves the five out.  Boundary vertices
        carry the value 0.  COLLECTIVE and independent of the number of ranks, bit for bit: a
        rank evaluates the nodes it owns, the sums over the mesh have one shape fixed by the
        number of cells, and one all-reduce with one non-zero contributor per entry gives
        every rank all of it.  A NaN threshold raises ValueError before anything touches the
        GPU; the plan is built by the first call (``curves_plan``), a run that never asks
        builds nothing.  Test-space vectors are refused.  Out of scope: time windows other than
        the nodes of [0, T], several thresholds in one call, sub-regions of the domain, values
        between the nodes.  The serial driver also takes `u` as a flat NumPy vector or a device
        vector and returns the same dict."""
        from .time_curves import check_arguments, time_curves
        check_arguments(threshold)  # before an upload or a plan
        return time_curves(self, self._trial_vector(u, 'time_curves()'), threshold)

    def solidification_maps(self, u, threshold, points=None, fields=None):
        """What a trial-space vector `u` (KronVectorMPI) does at the freezing front, per CELL of
        the mesh in the mesh's cell order, from one scan over the cells' rows on the device
        (source/solidification.py, csrc/solid.hip): a dict of device tensors 't_solid' and
        'cooling_rate' ((nc,): the last time the cell's mean dropped from above `threshold` to
        it or below, and -d/dt of the mean there; NaN if never), 'grad_solid' ((nc, d): grad
        u_h at that time), 'G' (its length, the square root taken in torch), 'front_speed'
        (cooling_rate / G: whatever IEEE gives where G == 0), 'n_solid' (int64: the number of
        such crossings, re-melts + 1), 'max_grad' and 't_max_grad' (the largest |grad u_h| over
        [0, T] -- exact, |grad u_h|^2 being a convex quadratic in t per element -- and the
        earliest node that has it).  A mean AT the threshold is not above, the rule of
        ``history_maps``.  `fields`: a subset of the names.  With `points` (n_p, d) -- NumPy
        array, device tensor or what ``sample_plan.locate`` returned --: the fields of the
        cell that holds each point plus 'inside'; NaN, and -1 for 'n_solid', outside the mesh
        (a gather by cell; no second scan).  COLLECTIVE and independent of the number of ranks,
        bit for bit: the scan's state travels down the ranks in time order (size - 1 transfers
        of 8 (6 + 2 d) nc bytes, serial by design).  A missing or NaN threshold, a wrong shape
        or an unknown field raises ValueError before anything touches the GPU; the plan is
        built by the first call (``solid_plan``).  Test-space vectors are refused.  Out of
        scope: per-cell thresholds, several thresholds in one call, melting crossings, time
        windows other than [0, T], a parallel merge of per-rank states.  The serial driver also
        takes `u` as a flat NumPy vector or a device vector and returns the same dict."""
        from .solidification import check_arguments, solidification_maps
        check_arguments(threshold, points, self._sample_meshes[0].points.shape[1], fields)  # before an upload or a plan
        u = self._trial_vector(u, 'solidification_maps()')
        if points is not None:
            self._sample_plan()
        return solidification_maps(self, u, threshold, points, fields)

    def isotherms(self, u, threshold, nodes=None, max_bytes=2**30):
        """The isotherm {u_h = threshold} of a trial-space vector `u` (KronVectorMPI) at the time
        nodes `nodes` (None: all N; or strictly ascending ints in [0, N)), as the segments (d =
        2) or triangles (d = 3) in which it cuts the cells -- exact for the P1 function, the cut
        of the zone of ``time_curves`` (source/isotherms.py, csrc/iso.hip): a dict of device
        tensors 'nodes' ((n_k,) int64) and 'times' ((n_k,), float(k) * h), 'offsets' ((n_k + 1,)
        int64: the pieces of nodes[k] are the rows offsets[k] .. offsets[k + 1]), 'vertices'
        ((n, d, d): the d vertices of a piece), 'grad' ((n, d): grad u_h in the piece's cell;
        the orientation of a piece is not promised, this orients it), 'cell' ((n,) int64),
        'measure' ((n,): the length or area of a piece, the square root taken in torch),
        'measure_at' ((n_k,): the length or area of the isotherm) and 'flux_at' ((n_k,): the sum
        of measure |grad u_h|, the heat crossing the isotherm per unit conductivity).  The
        pieces of a node come in the mesh's cell order.  A vertex AT the threshold is not above,
        the rule of ``time_curves``; boundary vertices carry the value 0; +-inf gives no piece.
        COLLECTIVE and independent of the number of ranks, bit for bit: a rank counts and fills
        the nodes it owns, the places of the records come from an exclusive scan of the int64
        counts per (node, tile of 256 cells), no atomics, the per-node sums are trees of one
        fixed shape, and two all-reduces with one non-zero contributor per entry give every
        rank all of it.  A missing or NaN threshold or bad `nodes` raises ValueError before
        anything touches the GPU; so does, before anything is allocated, a result of more than
        `max_bytes` bytes, naming the number of pieces.  The plan is the one of ``time_curves``
        (``curves_plan``), built by the first call of either.  Test-space vectors are refused.
        Out of scope: times between the nodes, several thresholds in one call, joining the
        pieces into polylines, orientation, sub-regions of the domain.  The serial driver also
        takes `u` as a flat NumPy vector or a device vector and returns the same dict."""
        from .isotherms import check_arguments, isotherms
        check_arguments(threshold, nodes, self._sample_meshes[1].nv, max_bytes)  # before an upload or a plan
        return isotherms(self, self._trial_vector(u, 'isotherms()'), threshold, nodes, max_bytes)

    def error_norms(self, u, exact=None, exact_grad=None, times=None):
        """|| u - u_h || of a trial-space vector `u` (KronVectorMPI) against `exact`
        (t, x, y[, z]) -- a pointwise function of float64 tensors that broadcast, evaluated on
        the device; default: the problem's data['exact'] -- in L2(I; L2), in L2(I; H^1_0) if
        `exact_grad` (default data['exact_grad'] when `exact` is the default too) is given, and
        in L2(Omega) at `times` (default [T]), by quadrature on the device
        (source/error_norms.py, csrc/err_norms.hip).  Returns a dict: l2_l2, l2_h1,
        exact_l2_l2, exact_l2_h1 (the norms of u by the same rule, for relative errors), l2_at
        (array over times) and per_element ((N - 1, 4) squares); H1 entries None without a
        gradient.  COLLECTIVE: every rank integrates the time elements whose upper node it
        owns and the per-element numbers are all-reduced with one contributor each, so every
        entry is the one-rank double whatever the number of ranks.  The plan is built by the
        first call; a run that never asks builds nothing.  The serial driver also takes `u` as a
        flat NumPy vector or a device vector and returns the same dict."""
        from .error_norms import ErrorPlan, error_norms_collective
        u = self._trial_vector(u, 'error_norms()')
        if exact is None:
            exact, default_grad = self._exact
            exact_grad = default_grad if exact_grad is None else exact_grad
        assert exact is not None, 'this problem has no exact solution: pass exact='
        return error_norms_collective(self._lazy_plan('error_plan', ErrorPlan), u, exact, exact_grad, times)

    def prolong_from(self, coarse_heat, u_coarse):
        """P u_c: the trial-space vector `u_coarse` of the COARSER discretisation `coarse_heat`
        (a driver object of this class on (J_time - a, J_space - s), a, s >= 0, built on the
        same communicator) as a trial-space vector of THIS discretisation that represents the
        same function -- P1 in space on the nested meshes, piecewise linear in time -- from one
        pass on the device (source/transfer.py, csrc/transfer.hip): a fine row copies its coarse
        row or is (A + B) * 0.5 of its two parents' values (0.0 on the boundary), a fine node
        k = (q << a) + rem is s(q), or (1.0 - rem / 2^a) * s(q) + (rem / 2^a) * s(q + 1), every
        operation rounded on its own.  Returns a new KronVectorMPI on this driver's
        distribution: the start of a nested iteration (``solve(x0=...)``), and with
        ``time_curves(u - P u_c)['l2_sq']`` the distance || u_h - P u_2h || of two levels.
        COLLECTIVE and independent of the number of ranks, bit for bit: every rank's coarse
        columns go into one (M_c, N_c) buffer, one all-reduce with one non-zero contributor per
        entry gives every rank all of it, and every rank prolongs into the columns it owns.
        Meshes that are not nested -- the coarse points, boundary flags and parents must be the
        prefix of the fine ones, T the same, the time elements in a ratio 2^a, a <= 8 -- raise
        ValueError before anything touches the GPU.  The plan is cached per coarse
        discretisation (``transfer_plans``) and built by the first call; a run that never asks
        builds nothing.  The adjoint is ``restrict_to``.  Out of scope: injection, test-space
        vectors, a neighbour-only exchange of the coarse columns, other time ratios, different
        coarsest meshes.  The serial driver also takes `u_coarse` as a flat NumPy vector or a
        device vector and returns a device vector (source.linop.host_vector copies it out;
        ``solve(x0=...)`` takes it as it is)."""
        from .transfer import prolong_from
        return prolong_from(self, coarse_heat, u_coarse)

    def restrict_to(self, coarse_heat, f):
        """P^T f: the FUNCTIONAL `f` on this discretisation's trial space (a right-hand side, a
        residual f - S u, what ``sample_along_adjoint`` returned) as the functional on the trial
        space of the COARSER discretisation `coarse_heat` with (P^T f) . v = f . (P v) for P of
        ``coarse_heat -> self`` (``prolong_from``) -- from one gather pass on the device
        (source/transfer.py, csrc/transfer.hip): a coarse row folds its own fine row (weight 1.0)
        and its children (0.5) in ascending fine row, then the 2^(a+1) - 1 fine nodes around its
        time node in ascending order with prolong's weights, every operation rounded on its own,
        no atomics.  Returns a new KronVectorMPI on `coarse_heat`'s distribution: the right-hand
        side of the coarse levels of a nested solve for a functional (``solve_nested(rhs=)``), and
        E_c^T = P^T E_f^T for point data.  COLLECTIVE and independent of the number of ranks, bit
        for bit: the last space level acts on every rank's own columns, one all-reduce with one
        non-zero contributor per entry, then the time stage and the remaining levels on the
        coarse columns a rank owns.  The checks and the plan cache are those of ``prolong_from``
        (``transfer_plans``); meshes that are not nested raise ValueError before anything touches
        the GPU; the transposed tables are built by the first restriction, a run that never
        restricts builds nothing of them.  Out of scope: injection, test-space vectors, a
        neighbour-only exchange, other time ratios.  The serial driver also takes `f` as a flat
        NumPy vector or a device vector."""
        from .transfer import restrict_to
        return restrict_to(self, coarse_heat, f)
