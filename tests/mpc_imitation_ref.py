"""CPU restatement of the MPC and Imitation action spaces in plain Python floats: what ``trajectory_tracking_mpc``
(smarts_amd/csrc/smx_vehicle.h) and ``k_control_kinematic<SMX_ACTION_SPACE_IMITATION>`` (smarts_amd/csrc/smx_kernels.hip)
compute, operation by operation.  Test infrastructure; held to the reference's own outputs
(tests/golden/mpc_cases.npz, tests/golden/imitation_cases.npz) by tests/test_mpc_imitation_cpu.py."""
import math

from kinematic_ref import heading_of, radians_to_vec

TWO_PI = 2 * math.pi
HORIZON = 5
# the sedan: chassis link mass and yaw inertia (models/vehicle.urdf), tyre cornering stiffnesses
# (models/tire_parameters.yaml), half the chassis length
MASS, INERTIA_Z, C_FRONT, C_REAR, HALF_LENGTH = 2356.0, 2681.95008628, 25000.0, 25000.0, 0.5 * 3.68


def clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def min_angles_difference_signed(first, second):
    return ((first - second) + math.pi) % TWO_PI - math.pi


def signed_dist_to_line(px, py, lx, ly, dx, dy):
    p2x, p2y = lx + dx, ly + dy
    u = abs(dy * px - dx * py + p2x * ly - p2y * lx)
    d = u / math.sqrt(dx * dx + dy * dy)
    dot = (px - lx) * -dy + (py - ly) * dx
    return d * (1.0 if dot > 0 else (-1.0 if dot < 0 else 0.0))


def curvature(tr, offset=0, num_points=5):
    """curvature_calculation (trajectory_tracking_controller.py:444-473)."""
    if len(tr[2]) <= num_points + offset:
        return 1e20
    hs = ds = 0.0
    for i in range(num_points):
        hs += min_angles_difference_signed(tr[2][i + 1 + offset], tr[2][i + offset])
        ex, ey = tr[0][i + offset] - tr[0][i + offset + 1], tr[1][i + offset] - tr[1][i + offset + 1]
        ds += abs(math.sqrt(ex * ex + ey * ey))
    return 1e20 if hs == 0 else ds / hs


class MpcState:
    """The three TrajectoryTrackingControllerState fields the MPC law updates, and the steer motor's target."""

    def __init__(self, velocity_error=0.0, integral_windup_error=0.0, throttle_state=0.0, steer=0.0):
        self.velocity_error, self.integral_windup_error, self.throttle_state = velocity_error, integral_windup_error, throttle_state
        self.steer = steer


def body_speeds(heading, u, v):
    """speed and (longitudinal, lateral) speed as the chassis reads them back from the world velocity
    (chassis.py:558-566) of a body with forward speed u and leftward speed v."""
    sh, ch = math.sin(heading), math.cos(heading)
    vx, vy = u * -sh + v * -ch, u * ch + v * -sh
    return math.sqrt(vx * vx + vy * vy + 0.0 * 0.0), vy * ch - vx * sh, vy * sh + vx * ch


def trajectory_tracking_mpc(tr, x, y, heading, speed, lng, lat, st, dt):
    """perform_trajectory_tracking_MPC (:56-173): ``tr`` = (xs, ys, headings, speeds) (any sequences: a packed
    trajectory indexes like the full one), the vehicle's pose, speed and longitudinal / lateral speed, ``st`` an
    MpcState (updated).  Returns (throttle, brake, steering)."""
    n = len(tr[2])
    ahead = abs(curvature(tr, 4))
    # ---- calculate_heading_lateral_error(initial_look_ahead_distant=3, speed reduction on)
    heading_error = min_angles_difference_signed(heading % TWO_PI, tr[2][0])
    look, look_dist = (1, 1.0) if ahead < 30 else (3, 3.0)
    k = min(look, n - 1)
    pvx, pvy = radians_to_vec(tr[2][k])
    lx, ly = x - look_dist * math.sin(heading), y + look_dist * math.cos(heading)
    lateral_error = signed_dist_to_line(lx, ly, tr[0][k], tr[1][k], pvx, pvy)
    # ---- calculate_raw_throttle_feedback(velocity_gain=1, traction_gain=8, throttle_filter_constant=10, the rest 0)
    desired = tr[3][n - 1]
    if ahead < 30:
        desired = clip(0.8 * desired, 0.0, 8.3)
    elif ahead < 100:
        desired *= 0.8
    velocity_error = speed - desired
    damping = (velocity_error - st.velocity_error) / dt
    raw = 3.6 * (-0.5 * 1.0 * velocity_error - 0.0 * (0.0 + 0.0 * st.integral_windup_error) - 0.0 * damping)
    st.velocity_error = velocity_error
    st.integral_windup_error = clip(raw, -1.0, 1.0) - raw
    prev = st.throttle_state + dt * 10.0 * (raw - st.throttle_state)
    st.throttle_state = clip(prev + -8.0 * abs(lat), -1.0, 1.0)
    if st.throttle_state > 0:
        brake, throttle = 0.0, clip(st.throttle_state, 0.0, 1.0)
    else:
        brake, throttle = clip(-st.throttle_state, 0.0, 1.0), 0.0
    # ---- MPC (:523-609) in closed form
    L, M, IZ, CF, CR = HALF_LENGTH, MASS, INERTIA_Z, C_FRONT, C_REAR
    v = max(0.1, lng)
    a11, a12, a13 = 1.0 + dt * (-(CF + CR) / (M * v)), 0.0 + dt * ((CF + CR) / M), 0.0 + dt * (L * (CF + CR) / (M * v))
    a31, a32, a33 = (0.0 + dt * (L * (-CF + CR) / (M * v)), 0.0 + dt * (L * (CF - CR) / M),
                     1.0 + dt * ((L * L) * (CF - CR) / (M * v)))

    def mul_a(p):
        return (p[0] + dt * p[1], a11 * p[1] + a12 * p[2] + a13 * p[3], p[2] + dt * p[3], a31 * p[1] + a32 * p[2] + a33 * p[3])

    q0, q2, q3 = 0.1 * 354.0, 0.1 * 14.0, 0.1 * 250.0

    def dot_q(p, r):
        return q0 * p[0] * r[0] + q2 * p[2] * r[2] + q3 * p[3] * r[3]

    g = [(0.0, dt * (CF / M), 0.0, dt * (CR / IZ))]
    for _ in range(1, HORIZON):
        g.append(mul_a(g[-1]))
    inv_curvature = 1.0 / curvature(tr, 0)
    x0 = (lateral_error, 0.0, heading_error, 0.0)
    td = (dt * (inv_curvature * 0.0), dt * (inv_curvature * ((L * CF + L * CR) / M - lng * lng)), dt * (inv_curvature * 0.0),
          dt * (inv_curvature * (((L * L) * CF - (L * L) * CR) / IZ)))
    z = []
    for k in range(HORIZON):
        x0 = mul_a(x0)
        if k > 0:
            td = mul_a(td)
        z.append(tuple(x0[c] + td[c] for c in range(4)))
    rhs = []
    for i in range(HORIZON):
        acc = 0.0
        for k in range(i, HORIZON):
            acc += dot_q(g[k - i], z[k])
        rhs.append(acc)
    gram = [[dot_q(g[a], g[b]) for b in range(a + 1)] for a in range(HORIZON)]
    H2 = [[0.0] * HORIZON for _ in range(HORIZON)]
    for i in range(HORIZON):
        for j in range(i + 1):
            acc = 0.0
            for k in range(i, HORIZON):
                acc += gram[k - j][k - i]
            H2[i][j] = 2.0 * (acc + (1.0 if i == j else 0.0))
    for p in range(HORIZON - 1, 0, -1):
        inv_pivot = 1.0 / H2[p][p]
        for i in range(p):
            f = H2[p][i] * inv_pivot
            for j in range(i + 1):
                H2[i][j] -= f * H2[p][j]
            rhs[i] -= f * rhs[p]
    u0 = rhs[0] / H2[0][0]
    steering = -clip(-u0, -1.0, 1.0)
    st.steer = steering
    return throttle, brake, steering


def imitation_step(x, y, heading, speed, act0, act1, dt):
    """ImitationController.perform_action on a BoxChassis (imitation_controller.py:50-78) for the action floats
    (act0, act1): the new (x, y, heading, speed), or None when the agent is not stepped (no action: NaN act0; or an
    action the device reports instead of carrying on: an infinite component, a pose or speed that is not finite)."""
    if act0 != act0:
        return None
    if act1 != act1:  # the scalar form: vehicle.control(vehicle.pose, action, dt)
        out = (x, y, heading, act0)
    else:
        if not (math.isfinite(act0) and math.isfinite(act1)):
            return None
        target = (heading + act1 * dt) % TWO_PI
        hvx, hvy = radians_to_vec(heading)
        qz, qw = math.sin(target * 0.5), math.cos(target * 0.5)
        yaw = math.atan2(2.0 * (0.0 * 0.0 + qw * qz), qw * qw + 0.0 * 0.0 - 0.0 * 0.0 - qz * qz)
        out = (x + hvx * speed * dt, y + hvy * speed * dt, heading_of(yaw), speed + act0 * dt)
    return out if all(math.isfinite(c) for c in out) else None
