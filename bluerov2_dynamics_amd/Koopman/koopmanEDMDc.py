"""EDMDc Koopman identification with an RBF dictionary -- drop-in for the reference's
Koopman/koopmanEDMDc.py (class KoopmanEDMDc: fit, fit_multi, evaluate, multistep_rmse, simulate,
_lift, _lift_inverse; dataclass fields state_dim, input_dim, n_rbfs, gamma, ridge, centers_, A_, B_,
lift_dim_).

What runs where:
  * RBF centres: the reference calls sklearn KMeans(n_clusters, n_init="auto", random_state=0) (:85,126).
    Here both halves run on the GPU (csrc/kmeans.hip): the k-means++ seeding restates scikit-learn's
    `_kmeans_plusplus` and consumes numpy's RandomState(0) in scikit-learn's order (engine.kmeanspp_draws,
    edmdc_kmeanspp_dev: same seed indices), then Lloyd's E/M loop with scikit-learn's stopping rules: same centres
    to rounding, tested.  `kmeans="sklearn"` calls scikit-learn for the whole thing instead;
  * lift phi(x) = [x, exp(-gamma(|x|^2+|c|^2-2x.c))] and the G^T[G|Y] normal-equation blocks:
    HIP kernels (csrc/edmdc.hip, fp64 MFMA);
  * the p x p ridge solve: on the host, numpy.linalg.pinv like the reference -- replaced by a symmetric eigendecomposition with the same
    cut-off only when the matrix is comfortably conditioned (pinv="auto", engine._host_pinv; measured against the reference's scores in
    tests/test_gpu_parity.py::test_fit_keeps_the_references_own_product_order and ::test_fit_at_class_defaults_with_a_wide_kernel).
    fit_multi associates M = pinv(G^T G + ridge I) (G^T Y) (:147) and so
    does fit_multi here; fit() evaluates (pinv G^T) Y left to right (:97) and so does fit() here (two more MFMA passes:
    rows of W = G P^T, then W^T Y).  The two differ by the conditioning of the Gram -- 1e-6 in the H = 100 RMSE at the
    class defaults (k = 200, ridge = 1e-8) -- which is why each method keeps its own order;
  * evaluate / multistep_rmse / simulate: H-step propagation Z <- Z A^T + U B^T as fp64 MFMA GEMMs
    (csrc/propagate.hip).
Unlike the reference, importing this module does not set OMP_NUM_THREADS / LOKY_MAX_CPU_COUNT.
Like the reference's module (numpy + scikit-learn only, Koopman/koopmanEDMDc.py:17,26-30), this one needs no torch: the library is
bound through ctypes and device memory comes from its own C ABI (engine.DevArray); torch is imported only if the caller asks for
arrays="torch" / pinv="device" or has imported it already (see _lib._one_hip_runtime).
"""
from dataclasses import dataclass

import numpy as np

from .. import engine


def _rbf_mat(X, C, gamma):
    """RBF feature matrix exp(-gamma |x - c|^2) in the reference's expanded form (Koopman/koopmanEDMDc.py:41-48):
    X [N,n], C [k,n] -> [N,k], evaluated by the lift kernel."""
    X = np.atleast_2d(np.asarray(X, dtype=float))
    C = np.atleast_2d(np.asarray(C, dtype=float))
    return engine.lift(X, C, float(gamma))[:, X.shape[1]:]


def _rbf(x, c, gamma):
    """One RBF value (Koopman/koopmanEDMDc.py:37-39)."""
    return float(_rbf_mat(np.asarray(x, dtype=float)[None, :], np.asarray(c, dtype=float)[None, :], gamma)[0, 0])


def _kmeans_centers(X, n_rbfs, backend="hip"):
    if backend == "sklearn":
        from sklearn.cluster import KMeans
        return KMeans(n_clusters=n_rbfs, n_init="auto", random_state=0).fit(X).cluster_centers_
    return engine.kmeans_centers(X, n_rbfs, random_state=0)


@dataclass
class KoopmanEDMDc:
    state_dim: int
    input_dim: int
    n_rbfs: int = 200
    gamma: float = 1.0
    ridge: float = 1e-8

    centers_: np.ndarray = None
    A_: np.ndarray = None
    B_: np.ndarray = None
    lift_dim_: int = None
    kmeans: str = "hip"                 # "hip" (k-means++ seeding and Lloyd on the GPU) or "sklearn"
    pinv: str = "auto"                  # the p x p solve (engine._host_pinv): "auto" = numpy.linalg.pinv like the reference (:97) unless G^T G + ridge I
                                        # is comfortably conditioned (then a symmetric eigendecomposition: same scores to 1e-10, half the time);
                                        # "host" = numpy.linalg.pinv always; "eigh" = the eigendecomposition always (speed, opt-in)
    arrays: str = "native"              # device-resident operands of fit / fit_multi: "native" = engine.DevArray through the C ABI (no torch),
                                        # "torch" = torch CUDA tensors (same launches, same bits)

    # ------------------------------------------------------------------ fitting
    def fit(self, X, U, centers=None) -> None:
        """Learn (A, B) from one rollout X (N,n), U (N,r) (reference :72-103).
        `centers` (k,n) overrides the KMeans step (extension, used for parity runs)."""
        if isinstance(X, engine.DevArray) or engine._is_torch(X):
            return self._fit_resident(X, U, centers)
        X = np.asarray(X, dtype=float)
        U = np.asarray(U, dtype=float)
        N, n = X.shape
        assert U.shape[0] == N and U.shape[1] == self.input_dim
        if N < 2 or (centers is None and self.kmeans == "sklearn"):
            self.centers_ = _kmeans_centers(X, self.n_rbfs, self.kmeans) if centers is None else np.asarray(centers, dtype=float)
            self._solve([X], [U], fit_order=True)
            return
        # one upload of the samples; centres, Gram and the two products of (P G^T) Y all read them where they lie in HBM
        # (round 2 uploaded X three times and went through three host entry points).  No torch on this path (round 6): the
        # buffers are brov_malloc'ed, the copies and launches go through the C ABI on the ctx's own stream.
        ctx = engine.default_context()
        ns = self._arrays(ctx)
        Xd = ns.upload(X)
        Ud = ns.upload(U[:N - 1])
        Cd = None if centers is None else ns.upload(np.asarray(centers, dtype=float))
        k = self.n_rbfs if centers is None else Cd.shape[0]
        self.A_, self.B_, C = engine.fit_dev(Xd, Ud, 1, N - 1, k, self.gamma, self.ridge, order="fit", centers=Cd, ctx=ctx, pinv=self.pinv)
        self.centers_ = ns.download(C) if centers is None else np.asarray(centers, dtype=float)
        self.lift_dim_ = self.state_dim + self.centers_.shape[0]

    def _fit_resident(self, Xd, Ud, centers):
        """fit() on samples that already live in HBM (engine.DevArray or torch CUDA tensors [N,n] / [N,r] or [N-1,r]: e.g.
        data.load_dataset_dev, a simulated ensemble): the same pipeline without the upload; the inputs' last row is never read."""
        if engine._is_torch(Xd):                    # (a tensor made from a Fortran-ordered array -- pandas' to_numpy -- has strided rows)
            Xd, Ud = Xd.contiguous(), Ud.contiguous()
        N = Xd.shape[0]
        assert Xd.shape[1] == self.state_dim and Ud.shape[1] == self.input_dim and Ud.shape[0] >= N - 1 and N >= 2
        ctx = engine._ctx_of(Xd, None)
        ns = engine.arrays_of(Xd, ctx)
        if centers is None and self.kmeans == "sklearn":          # scikit-learn picks the centres on the host, the device does the rest
            centers = _kmeans_centers(ns.download(Xd), self.n_rbfs, "sklearn")
        Cd = None if centers is None else ns.upload(np.asarray(centers, dtype=float))
        k = self.n_rbfs if centers is None else Cd.shape[0]
        self.A_, self.B_, C = engine.fit_dev(Xd, Ud, 1, N - 1, k, self.gamma, self.ridge, order="fit", centers=Cd, ctx=ctx, pinv=self.pinv)
        self.centers_ = ns.download(C) if centers is None else np.asarray(centers, dtype=float)
        self.lift_dim_ = self.state_dim + self.centers_.shape[0]

    def _arrays(self, ctx):
        """where fit / fit_multi keep their device-resident operands: engine.DevArray (default; no torch anywhere) or torch CUDA tensors
        (arrays="torch", and always for pinv="device", which is torch.linalg.eigh) -- the same kernels with the same arguments."""
        if self.arrays == "torch" or self.pinv == "device":
            return engine._TorchArrays(ctx)
        if self.arrays != "native":
            raise ValueError("arrays must be 'native' or 'torch'")
        return engine._NativeArrays(ctx)

    def fit_multi(self, X_list, U_list, centers=None) -> None:
        """Fit from several independent trajectories without cross-bag transitions (reference :113-152).  The list may be ragged
        (any lengths; bags with fewer than two states contribute no pair, :131-132, but their states are clustered, :125).
        The whole list is uploaded ONCE, bag by bag into one device buffer (engine.upload_bags: no stacked copy on the host); k-means,
        the ragged Gram (edmdc_gram_ragged_dev) and the solve run on that resident copy, whatever the number of bags."""
        assert len(X_list) == len(U_list) and len(X_list) > 0
        n, r = self.state_dim, self.input_dim
        for X, U in zip(X_list, U_list):
            assert X.shape[1] == n and U.shape[1] == r
        ctx = engine.default_context()
        ns = self._arrays(ctx)
        Xd, Ud, off = engine.upload_bags(X_list, U_list, n, r, ctx=ctx, arrays=ns.kind)
        lens = np.diff(off)
        if off[-1] == 0 or not (lens >= 2).any():
            # np.vstack of an empty list (reference :125 when every bag is empty, :140 when no bag holds a pair)
            raise ValueError("need at least one array to concatenate")
        if centers is None and self.kmeans == "sklearn":
            centers = _kmeans_centers(ns.download(Xd), self.n_rbfs, "sklearn")
        Cd = None if centers is None else ns.upload(np.asarray(centers, dtype=float))
        k = self.n_rbfs if centers is None else Cd.shape[0]
        self.A_, self.B_, C = engine.fit_dev(Xd, Ud, 0, 0, k, self.gamma, self.ridge, order="fit_multi", centers=Cd, ctx=ctx, pinv=self.pinv,
                                             bag_offsets=off)
        self.centers_ = ns.download(C) if centers is None else np.asarray(centers, dtype=float)
        self.lift_dim_ = self.state_dim + self.centers_.shape[0]

    def _solve(self, X_list, U_list, fit_order=False):
        GtG, GtY, _ = engine.gram(X_list, U_list, self.centers_, self.gamma)
        d = self.state_dim + self.centers_.shape[0]
        if fit_order:       # (pinv G^T) Y, Koopman/koopmanEDMDc.py:97
            self.A_, self.B_ = engine.solve_AB_fit_order(X_list, U_list, self.centers_, self.gamma, GtG, self.ridge, d, pinv=self.pinv)
        else:               # pinv (G^T Y), :147
            self.A_, self.B_ = engine.solve_AB(GtG, GtY, self.ridge, d, pinv=self.pinv)
        self.lift_dim_ = d

    # ------------------------------------------------------------------ scoring
    def evaluate(self, X, U) -> float:
        """One-step RMSE in state space (reference :157-170)."""
        return self.multistep_rmse(X, U, H=1)

    def multistep_rmse(self, X, U, H: int = 10, method: str = "propagate") -> float:
        """RMSE after H open-loop steps from every start index (reference :172-200).  method="propagate" (default): H lifted steps
        Z <- Z A^T + U_t B^T like the reference; "linear" (opt-in): the same prediction through the explicit powers of A in one pass
        over the windows (engine.multistep_se_linear) -- equal to rounding, ~40 x less arithmetic at H = 100."""
        X = np.asarray(X, dtype=float)
        n_start = len(X) - H
        if hasattr(self, "decoder_"):
            raise NotImplementedError("decoder_ is never set by the reference's fit(); not supported")
        if method == "propagate":
            se, _ = engine.multistep_se(X, U, self.centers_, self.gamma, self.A_, self.B_, H)
        elif method == "linear":
            se, _ = engine.multistep_se_linear(X, U, self.centers_, self.gamma, self.A_, self.B_, H)
        else:
            raise ValueError("method must be 'propagate' or 'linear'")
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(np.sqrt(np.float64(se) / (n_start * X.shape[1]))) if n_start > 0 else float("nan")

    def simulate(self, x0, U_seq) -> np.ndarray:
        """Open-loop prediction (T+1, n) (reference :202-216)."""
        x0 = np.asarray(x0, dtype=float)
        U_seq = np.asarray(U_seq, dtype=float).reshape(-1, self.input_dim)
        return engine.simulate_lifted(x0[None], U_seq[None], self.centers_, self.gamma, self.A_, self.B_)[0]

    def mppi_planner(self, H, hold=1, ctx=None):
        """The fitted model made ready for model-predictive control over a horizon of H steps with `hold` steps per knot
        (engine.KoopmanPlanner): centres, A, B and the coefficients of the linear-in-the-command predictor are uploaded once.  The
        model is taken to be fitted at the planning step (one row of the recording per step).  planner.step(cfg, x, ref, U_nom, dt,
        K) is one update (engine.koopman_mppi_step); VehicleBase.simulate_mppi(..., planner=planner) plans every tick with it."""
        if self.A_ is None or self.B_ is None or self.centers_ is None:
            raise ValueError("fit the model first: mppi_planner needs centers_, A_ and B_")
        return engine.KoopmanPlanner(self.centers_, self.gamma, self.A_, self.B_, H, hold, ctx=ctx)

    def lmpc_planner(self, H, cfg, dt, ctx=None):
        """The fitted model made ready for LINEAR model-predictive control (engine.KoopmanLmpc): the tracking problem over H steps of
        dt under the record cfg (fossen/control.py: lmpc) is a box-constrained QP in the knots, whose matrix is condensed and
        inverted once here; planner.step(x, ref, U_nom, y) solves it for a batch of states (engine.koopman_lmpc_step);
        VehicleBase.simulate_lmpc(..., planner=planner) plans every tick with it.  ValueError when the weights leave the QP
        without a unique minimum."""
        if self.A_ is None or self.B_ is None or self.centers_ is None:
            raise ValueError("fit the model first: lmpc_planner needs centers_, A_ and B_")
        return engine.KoopmanLmpc(self.centers_, self.gamma, self.A_, self.B_, H, cfg, dt, ctx=ctx)

    # ------------------------------------------------------------------ persistence (new: the reference never stores it)
    def save(self, path) -> None:
        np.savez(path, state_dim=self.state_dim, input_dim=self.input_dim, n_rbfs=self.n_rbfs, gamma=self.gamma, ridge=self.ridge,
                 centers_=self.centers_, A_=self.A_, B_=self.B_, lift_dim_=self.lift_dim_)

    @classmethod
    def load(cls, path) -> "KoopmanEDMDc":
        z = np.load(path, allow_pickle=False)
        m = cls(state_dim=int(z["state_dim"]), input_dim=int(z["input_dim"]), n_rbfs=int(z["n_rbfs"]), gamma=float(z["gamma"]),
                ridge=float(z["ridge"]))
        m.centers_, m.A_, m.B_, m.lift_dim_ = z["centers_"], z["A_"], z["B_"], int(z["lift_dim_"])
        return m

    # ------------------------------------------------------------------ helpers
    def _lift(self, x):
        """phi(x) = [x, RBF_1(x) .. RBF_k(x)] for (n,) or (N,n) input (reference :221-236)."""
        x = np.asarray(x, dtype=float)
        if x.ndim == 1:
            return engine.lift(x[None, :], self.centers_, self.gamma)[0]
        if x.ndim == 2:
            return engine.lift(x, self.centers_, self.gamma)
        raise ValueError("x must have ndim 1 or 2")

    def _lift_inverse(self, z):
        """First n coordinates of the lifted state (reference :238-248)."""
        if hasattr(self, "decoder_"):
            return z @ self.decoder_.T
        return z[..., :self.state_dim]
