"""NumPy restatement of the reference's visual-inertial fusion: SensorFusion (an error-state EKF over position, velocity,
orientation and the two IMU biases; include/legacy/IMU.hpp:53-118, src/legacy/IMU.cpp:102-305) and IMUPreintegrator
(IMU.hpp:17-51, IMU.cpp:28-100). This file IS THE DEFINITION of the stage that aria_slam_amd/csrc/imu_fusion.hip runs on the
device (include/aria_orb_hip.h, "visual-inertial fusion"). Eigen is not available to this project, so the reference classes
cannot be compiled here: PARITY WITH AN EIGEN BUILD IS NOT PINNED by any test. What is restated is what the code does,
including what looks odd:

- addIMU before the first visual pose does nothing to the state (the reference's deque is never read and is not kept here);
- the prediction uses R of the orientation BEFORE the gyro step for the acceleration and for F and G, advances the
  orientation on the right (q * dq), while the update applies its correction on the left (exp(dx) * q);
- F is not the exact Jacobian of the prediction (see tests/test_fuse_host.py: the orientation rows carry no dependence on
  the rotation itself, and dp/dba, dv/dba are those of the model, which the prediction follows exactly);
- the preintegrator rotates the acceleration by delta_q BEFORE a sample's rotation and builds F and G from delta_q AFTER it,
  never symmetrises its covariance, and stores a gravity vector that it never uses.

Three Eigen internals are written out and are ours by definition:
- quat_from_rot: the trace branch when trace > 0, otherwise the largest diagonal entry (the first of equals); the sign of w is
  NOT forced (graph_ref.quat_from_rot forces w >= 0). Nothing downstream depends on that sign: R(q), the products'
  normalisation and log_map are all invariant under q -> -q;
- log_map: through the angle-axis form, angle = 2 atan2(|vec|, |w|), axis = vec / |vec| negated when w < 0, the zero vector when
  |vec| = 0;
- S^-1 of the 6x6 innovation covariance: Cholesky (lower, no pivoting), applied as two triangular solves to (P H^T)^T. A pivot
  that is not > 0 skips the update (a rule of ours; the filter's own P never produces one).

Every function takes or inherits a `dtype`: the same code runs in np.longdouble, and that run is the yardstick of the
tolerances in tests/test_gpu_fuse.py."""
import numpy as np

H_IDX = (0, 1, 2, 6, 7, 8)      # rows of the error state the visual measurement sees: position and orientation


# ---- quaternions, (w, x, y, z) ---------------------------------------------------------------------------------------------
def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]], dtype=a.dtype)


def quat_normalize(q):
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def quat_inverse(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return np.array([q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2], dtype=q.dtype)


def quat_to_rot(q):
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = q.dtype.type(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=q.dtype)


def quat_from_rot(R):
    R = np.asarray(R)
    T = R.dtype.type
    half, one = T(0.5), T(1)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4, R.dtype)
    if tr > 0:
        s = np.sqrt(tr + one)
        q[0] = half * s
        s = half / s
        q[1] = (R[2, 1] - R[1, 2]) * s
        q[2] = (R[0, 2] - R[2, 0]) * s
        q[3] = (R[1, 0] - R[0, 1]) * s
        return q
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + one)
    q[1 + i] = half * s
    s = half / s
    q[0] = (R[k, j] - R[j, k]) * s
    q[1 + j] = (R[j, i] + R[i, j]) * s
    q[1 + k] = (R[k, i] + R[i, k]) * s
    return q


def quat_angle_axis(angle, v):
    """Quaternion of AngleAxis(angle, v / angle); the caller has checked angle."""
    h = v.dtype.type(0.5) * angle
    s, c = np.sin(h), np.cos(h)
    return np.array([c, s * (v[0] / angle), s * (v[1] / angle), s * (v[2] / angle)], dtype=v.dtype)


def exp_map(theta):
    angle = np.sqrt(theta[0] * theta[0] + theta[1] * theta[1] + theta[2] * theta[2])
    if angle < 1e-10:
        return np.array([1, 0, 0, 0], dtype=theta.dtype)
    return quat_angle_axis(angle, theta)


def log_map(q):
    n = np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if n == 0:
        return np.zeros(3, q.dtype)
    angle = 2 * np.arctan2(n, abs(q[0]))
    if q[0] < 0:
        n = -n
    return np.array([angle * (q[1] / n), angle * (q[2] / n), angle * (q[3] / n)], dtype=q.dtype)


def skew(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=v.dtype)


def cholesky_lower(S):
    """(L, ok): S = L L^T without pivoting; ok = False when a pivot is not > 0 (L is then meaningless)."""
    n = len(S)
    L = np.zeros_like(S)
    for a in range(n):
        for b in range(a + 1):
            s = S[a, b]
            for k in range(b):
                s = s - L[a, k] * L[b, k]
            if a == b:
                if not s > 0:
                    return L, False
                L[a, a] = np.sqrt(s)
            else:
                L[a, b] = s / L[b, b]
    return L, True


def cholesky_solve(L, B):
    """X with (L L^T) X = B, column by column: forward then backward substitution."""
    n = len(L)
    X = np.array(B, dtype=L.dtype, copy=True)
    for col in range(X.shape[1]):
        for a in range(n):
            s = X[a, col]
            for k in range(a):
                s = s - L[a, k] * X[k, col]
            X[a, col] = s / L[a, a]
        for a in range(n - 1, -1, -1):
            s = X[a, col]
            for k in range(a + 1, n):
                s = s - L[k, a] * X[k, col]
            X[a, col] = s / L[a, a]
    return X


# ---- SensorFusion ----------------------------------------------------------------------------------------------------------
DEFAULT_NOISE = dict(accel_noise=0.1, gyro_noise=0.01, accel_bias_walk=0.001, gyro_bias_walk=0.0001, pos_noise=0.01,
                     rot_noise=0.01)
DEFAULT_GRAVITY = (0.0, 0.0, -9.81)


def predict_jacobians(R, accel, dt):
    """The reference's F (15x15) and G (15x12) of one prediction (IMU.cpp:179-213): R is the rotation before the gyro step,
    accel the bias-free acceleration."""
    T = R.dtype.type
    I3 = np.eye(3, dtype=R.dtype)
    F = np.eye(15, dtype=R.dtype)
    RS = R @ skew(accel)
    F[0:3, 3:6] = I3 * dt
    F[0:3, 6:9] = ((T(-0.5) * RS) * dt) * dt
    F[0:3, 9:12] = ((T(-0.5) * R) * dt) * dt
    F[3:6, 6:9] = -RS * dt
    F[3:6, 9:12] = -R * dt
    F[6:9, 12:15] = -I3 * dt
    G = np.zeros((15, 12), R.dtype)
    G[0:3, 0:3] = ((T(0.5) * R) * dt) * dt
    G[3:6, 0:3] = R * dt
    G[6:9, 3:6] = I3 * dt
    G[9:12, 6:9] = I3 * dt
    G[12:15, 9:12] = I3 * dt
    return F, G


class SensorFusion:
    """The reference class's surface (add_imu, add_visual_pose, getters) over plain arrays."""

    def __init__(self, dtype=np.float64, gravity=DEFAULT_GRAVITY, **noise):
        self.dtype = np.dtype(dtype)
        T = self.dtype.type
        n = dict(DEFAULT_NOISE)
        n.update(noise)
        self.noise = {k: T(v) for k, v in n.items()}
        self.gravity = np.array(gravity, dtype=self.dtype)
        self.position = np.zeros(3, self.dtype)
        self.velocity = np.zeros(3, self.dtype)
        self.orientation = np.array([1, 0, 0, 0], dtype=self.dtype)
        self.accel_bias = np.zeros(3, self.dtype)
        self.gyro_bias = np.zeros(3, self.dtype)
        self.P = np.diag(np.array([0.01] * 9 + [0.001] * 3 + [0.0001] * 3, dtype=self.dtype))
        self.last_imu_time = T(-1)
        self.last_visual_time = T(-1)
        self.initialized = False
        # per-frame counters (the device's aria_fuse_state carries them); reset by run_track per frame
        self.n_predicted = self.n_skipped = self.n_ignored = self.n_updates = 0

    @property
    def Q(self):
        n = self.noise
        return np.diag(np.repeat(np.array([n[k] * n[k] for k in ("accel_noise", "gyro_noise", "accel_bias_walk",
                                                                     "gyro_bias_walk")], dtype=self.dtype), 3))

    @property
    def R_meas(self):
        n = self.noise
        return np.diag(np.repeat(np.array([n["pos_noise"] * n["pos_noise"], n["rot_noise"] * n["rot_noise"]], dtype=self.dtype), 3))

    # -- addIMU + predictEKF
    def add_imu(self, t, accel, gyro):
        if not self.initialized:
            self.n_ignored += 1
            return
        T = self.dtype.type
        t = T(t)
        if self.last_imu_time < 0:
            self.last_imu_time = t
            self.n_skipped += 1
            return
        dt = t - self.last_imu_time
        if dt <= 0 or dt > T(0.1):
            self.last_imu_time = t
            self.n_skipped += 1
            return
        self.n_predicted += 1
        a = np.asarray(accel, self.dtype) - self.accel_bias
        w = np.asarray(gyro, self.dtype) - self.gyro_bias
        R = quat_to_rot(self.orientation)
        d = w * dt
        angle = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        if angle > 1e-10:
            self.orientation = quat_normalize(quat_mul(self.orientation, quat_angle_axis(angle, d)))
        aw = np.array([(R[r, 0] * a[0] + R[r, 1] * a[1] + R[r, 2] * a[2]) + self.gravity[r] for r in range(3)],
                      dtype=self.dtype)
        self.position = self.position + (self.velocity * dt + ((T(0.5) * aw) * dt) * dt)
        self.velocity = self.velocity + aw * dt
        F, G = predict_jacobians(R, a, dt)
        P = F @ self.P @ F.T + G @ self.Q @ G.T
        self.P = T(0.5) * (P + P.T)
        self.last_imu_time = t

    # -- addVisualPose + updateEKF
    def add_visual_pose(self, t, R, p):
        T = self.dtype.type
        t = T(t)
        R = np.asarray(R, self.dtype).reshape(3, 3)
        p = np.asarray(p, self.dtype).reshape(3)
        if not self.initialized:
            self.position = p.copy()
            self.orientation = quat_from_rot(R)
            self.velocity = np.zeros(3, self.dtype)
            self.last_visual_time = t
            self.last_imu_time = t
            self.initialized = True
            return
        self._update(R, p)
        self.last_visual_time = t

    def _update(self, R, p):
        T = self.dtype.type
        h = list(H_IDX)
        S = self.P[np.ix_(h, h)] + self.R_meas
        L, ok = cholesky_lower(S)
        if not ok:
            return
        self.n_updates += 1
        q_err = quat_normalize(quat_mul(quat_from_rot(R), quat_inverse(self.orientation)))
        innov = np.concatenate([p - self.position, log_map(q_err)])
        K = cholesky_solve(L, self.P[:, h].T.copy()).T          # P H^T S^-1
        dx = np.array([sum(K[c, j] * innov[j] for j in range(6)) for c in range(15)], dtype=self.dtype)
        self.position = self.position + dx[0:3]
        self.velocity = self.velocity + dx[3:6]
        self.orientation = quat_normalize(quat_mul(exp_map(dx[6:9]), self.orientation))
        self.accel_bias = self.accel_bias + dx[9:12]
        self.gyro_bias = self.gyro_bias + dx[12:15]
        Hm = np.zeros((6, 15), self.dtype)
        for j, c in enumerate(h):
            Hm[j, c] = 1
        I_KH = np.eye(15, dtype=self.dtype) - K @ Hm
        P = I_KH @ self.P @ I_KH.T + K @ self.R_meas @ K.T
        self.P = T(0.5) * (P + P.T)

    # -- getters
    def get_position(self):
        return self.position.copy()

    def get_velocity(self):
        return self.velocity.copy()

    def get_orientation(self):
        return self.orientation.copy()

    def get_bias(self):
        return self.accel_bias.copy(), self.gyro_bias.copy()

    def get_covariance(self):
        return self.P.copy()

    def is_initialized(self):
        return self.initialized

    def astype(self, dtype):
        """A copy of the whole filter in another dtype."""
        o = SensorFusion(dtype, gravity=[float(g) for g in self.gravity], **{k: float(v) for k, v in self.noise.items()})
        for k in ("position", "velocity", "orientation", "accel_bias", "gyro_bias", "P"):
            setattr(o, k, getattr(self, k).astype(o.dtype))
        o.last_imu_time = o.dtype.type(self.last_imu_time)
        o.last_visual_time = o.dtype.type(self.last_visual_time)
        o.initialized = self.initialized
        return o


STATE_FIELDS = ("t", "p", "v", "q", "ba", "bg", "P_diag", "n_predicted", "n_skipped", "n_ignored", "n_updates", "initialized")


def run_track(flt, imu, imu_end, visual):
    """Feeds `flt` (a SensorFusion, updated in place) one track. imu: (N, 7) rows [t, accel, gyro]; imu_end: (F,) the sample
    count consumed up to and including frame f; visual: list of (t, R 3x3, p 3, accept). Frame f consumes the samples
    [imu_end[f-1], imu_end[f]), then its visual record when accepted (src/euroc_eval.cpp:139-142, :209). Returns the
    per-frame states as a dict of arrays (STATE_FIELDS)."""
    imu = np.asarray(imu)
    F = len(visual)
    dt = flt.dtype
    out = dict(t=np.zeros(F, dt), p=np.zeros((F, 3), dt), v=np.zeros((F, 3), dt), q=np.zeros((F, 4), dt),
               ba=np.zeros((F, 3), dt), bg=np.zeros((F, 3), dt), P_diag=np.zeros((F, 15), dt))
    for k in STATE_FIELDS[7:]:
        out[k] = np.zeros(F, np.int32)
    i = 0
    for f in range(F):
        flt.n_predicted = flt.n_skipped = flt.n_ignored = flt.n_updates = 0
        while i < int(imu_end[f]):
            flt.add_imu(imu[i, 0], imu[i, 1:4], imu[i, 4:7])
            i += 1
        t, R, p, accept = visual[f]
        if accept:
            flt.add_visual_pose(t, R, p)
        out["t"][f] = t
        out["p"][f], out["v"][f], out["q"][f] = flt.position, flt.velocity, flt.orientation
        out["ba"][f], out["bg"][f] = flt.accel_bias, flt.gyro_bias
        out["P_diag"][f] = np.diag(flt.P)
        out["n_predicted"][f], out["n_skipped"][f] = flt.n_predicted, flt.n_skipped
        out["n_ignored"][f], out["n_updates"][f] = flt.n_ignored, flt.n_updates
        out["initialized"][f] = int(flt.initialized)
    return out


# ---- IMUPreintegrator ------------------------------------------------------------------------------------------------------
class IMUPreintegrator:
    def __init__(self, gravity=DEFAULT_GRAVITY, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.gravity = np.array(gravity, dtype=self.dtype)     # stored and never used, as in the reference
        self.accel_noise = self.dtype.type(0.01)
        self.gyro_noise = self.dtype.type(0.001)
        self.accel_bias = np.zeros(3, self.dtype)
        self.gyro_bias = np.zeros(3, self.dtype)
        self.reset()

    def reset(self):
        T = self.dtype.type
        self.delta_p = np.zeros(3, self.dtype)
        self.delta_v = np.zeros(3, self.dtype)
        self.delta_q = np.array([1, 0, 0, 0], dtype=self.dtype)
        self.dt_sum = T(0)
        self.last_timestamp = T(-1)
        self.covariance = np.zeros((9, 9), self.dtype)
        self.n_used = 0

    def set_bias(self, accel_bias, gyro_bias):
        self.accel_bias = np.asarray(accel_bias, self.dtype).copy()
        self.gyro_bias = np.asarray(gyro_bias, self.dtype).copy()

    def integrate(self, t, accel, gyro):
        T = self.dtype.type
        t = T(t)
        if self.last_timestamp < 0:
            self.last_timestamp = t
            return
        dt = t - self.last_timestamp
        self.last_timestamp = t
        if dt <= 0 or dt > T(0.5):
            return
        self.n_used += 1
        a = np.asarray(accel, self.dtype) - self.accel_bias
        w = np.asarray(gyro, self.dtype) - self.gyro_bias
        d = w * dt
        angle = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        R = quat_to_rot(self.delta_q)
        aw = np.array([R[r, 0] * a[0] + R[r, 1] * a[1] + R[r, 2] * a[2] for r in range(3)], dtype=self.dtype)
        self.delta_p = self.delta_p + (self.delta_v * dt + ((T(0.5) * aw) * dt) * dt)
        self.delta_v = self.delta_v + aw * dt
        if angle > 1e-10:
            self.delta_q = quat_mul(self.delta_q, quat_angle_axis(angle, d))
        self.delta_q = quat_normalize(self.delta_q)
        R = quat_to_rot(self.delta_q)
        I3 = np.eye(3, dtype=self.dtype)
        F = np.eye(9, dtype=self.dtype)
        F[0:3, 3:6] = I3 * dt
        F[3:6, 6:9] = (-R @ skew(a)) * dt
        G = np.zeros((9, 6), self.dtype)
        G[3:6, 0:3] = R * dt
        G[6:9, 3:6] = I3 * dt
        Q = np.diag(np.repeat(np.array([self.accel_noise * self.accel_noise, self.gyro_noise * self.gyro_noise],
                                       dtype=self.dtype), 3))
        self.covariance = F @ self.covariance @ F.T + G @ Q @ G.T
        self.dt_sum = self.dt_sum + dt


def preintegrate(imu, begin, end, bias=None, dtype=np.float64):
    """Intervals [begin[i], end[i]) of imu (N, 7): dict of arrays delta_p, delta_v, delta_q, dt_sum, cov (n, 9, 9), n_used."""
    imu = np.asarray(imu)
    n = len(begin)
    dt = np.dtype(dtype)
    out = dict(delta_p=np.zeros((n, 3), dt), delta_v=np.zeros((n, 3), dt), delta_q=np.zeros((n, 4), dt), dt_sum=np.zeros(n, dt),
               cov=np.zeros((n, 9, 9), dt), n_used=np.zeros(n, np.int32))
    for k in range(n):
        pre = IMUPreintegrator(dtype=dtype)
        if bias is not None:
            pre.set_bias(bias[0:3], bias[3:6])
        for i in range(int(begin[k]), int(end[k])):
            pre.integrate(imu[i, 0], imu[i, 1:4], imu[i, 4:7])
        out["delta_p"][k], out["delta_v"][k], out["delta_q"][k] = pre.delta_p, pre.delta_v, pre.delta_q
        out["dt_sum"][k], out["cov"][k], out["n_used"][k] = pre.dt_sum, pre.covariance, pre.n_used
    return out


# ---- scene generator for the tests -----------------------------------------------------------------------------------------
def rot_zyx(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def rotvec_to_rot(r):
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.eye(3) + skew(np.asarray(r, np.float64))
    K = skew(np.asarray(r, np.float64) / th)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def make_scene(seed, duration=20.0, imu_rate=200.0, every=10, radius=2.0, period=10.0, wobble=0.3, accel_bias=(0.05, -0.03, 0.02),
               gyro_bias=(0.002, -0.001, 0.0015), accel_sigma=0.05, gyro_sigma=0.002, pos_sigma=0.01, rot_sigma=0.005, t0=100.0, yaw_follows=False):
    """A circle of `radius` metres with a vertical wobble, the body yawing with the tangent and pitching a little. The IMU runs
    at `imu_rate` Hz with constant biases and white noise; every `every` samples a visual pose with `pos_sigma` metres /
    `rot_sigma` radians of noise. Returns a dict: imu (N, 7), imu_end (F,), visual [(t, R, p, accept)], truth_p (F, 3),
    truth_R (F, 3, 3), meas_p (F, 3). Frame f's pose is taken at the time of its last sample. All fp64."""
    rng = np.random.default_rng(seed)
    n = int(round(duration * imu_rate))
    dt = 1.0 / imu_rate
    t = t0 + dt * np.arange(1, n + 1)
    om = 2 * np.pi / period
    s = t - t0

    def pose(s):
        p = np.array([radius * np.cos(om * s), radius * np.sin(om * s), wobble * np.sin(2 * om * s)])
        yaw = om * s + np.pi / 2 if yaw_follows else 0.2 * np.sin(om * s)
        R = rot_zyx(yaw, 0.1 * np.sin(om * s), 0.05 * np.cos(2 * om * s))
        return p, R

    imu = np.zeros((n, 7))
    h = 1e-4
    g = np.array(DEFAULT_GRAVITY)
    for k in range(n):
        # the sample at t[k] describes the motion over (t[k-1], t[k]]: evaluated at the interval's middle
        sm = s[k] - 0.5 * dt
        p0, R0 = pose(sm)
        pa, _ = pose(sm - h)
        pb, Rb = pose(sm + h)
        _, Ra = pose(sm - h)
        acc_w = (pa - 2 * p0 + pb) / (h * h)
        dR = Ra.T @ Rb
        w_b = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / (4 * h)
        imu[k, 0] = t[k]
        imu[k, 1:4] = R0.T @ (acc_w - g) + np.asarray(accel_bias) + accel_sigma * rng.standard_normal(3)
        imu[k, 4:7] = w_b + np.asarray(gyro_bias) + gyro_sigma * rng.standard_normal(3)
    # frame 0 sits at t0 with no sample before it; frame f >= 1 follows `every` samples
    F = n // every + 1
    imu_end = np.array([f * every for f in range(F)], np.int32)
    visual, truth_p, truth_R, meas_p = [], [], [], []
    for f in range(F):
        sf = (f * every) * dt
        p, R = pose(sf)
        pm = p + pos_sigma * rng.standard_normal(3)
        Rm = R @ rotvec_to_rot(rot_sigma * rng.standard_normal(3))
        visual.append((t0 + sf, Rm, pm, 1))
        truth_p.append(p)
        truth_R.append(R)
        meas_p.append(pm)
    return dict(imu=imu, imu_end=imu_end, visual=visual, truth_p=np.array(truth_p), truth_R=np.array(truth_R),
                meas_p=np.array(meas_p))
