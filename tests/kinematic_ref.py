"""CPU restatement of the kinematic action spaces (TargetPose, TrajectoryWithTime) and of BoxChassis' read-back, in
plain Python floats: what k_control_kinematic (smarts_amd/csrc/smx_k_control.h) and the kinematic ego read-back of the
observe role (smarts_amd/csrc/smx_k_observe.h) compute, operation by operation.  Test infrastructure; held to the
reference's own outputs (tests/golden/kinematic_*.npz) by tests/test_kinematic_cpu.py."""
import math

TWO_PI = 2 * math.pi


def heading_of(value):
    """Heading.__new__ (coordinates.py:175-184)."""
    value = value % TWO_PI
    if value > math.pi:
        value -= TWO_PI
    return value


def bezier_first_point(x, y, raw, target, dt):
    """MotionPlannerProvider.step for one vehicle (motion_planner_provider.py:85-99 ->
    bezier_motion_planner.py:53-121 with n = 1): the provider's new pose row (x, y, un-normalised heading) and the
    speed.  ``target`` = (x, y, heading, seconds) or None (no action: the pose held, dt ahead, :119-129)."""
    tx, ty, th, seconds = (x, y, raw, dt) if target is None else target
    target_heading, current_heading = th + math.pi * 0.5, raw + math.pi * 0.5
    tdir = (math.cos(target_heading), math.sin(target_heading))
    cdir = (math.cos(current_heading), math.sin(current_heading))
    ex, ey = tx - x, ty - y
    extension = math.sqrt(ex * ex + ey * ey) * 0.9
    p0, p3 = (x, y), (tx, ty)
    p1 = tuple(p0[q] + cdir[q] * extension * 0.5 for q in range(2))
    p2 = tuple(p3[q] - tdir[q] * extension * (1 - 0.5) for q in range(2))
    t = (1 * dt) / (dt if seconds < dt else seconds)

    def linear(a, b):
        return (1 - t) * a + t * b

    def quadratic(a, b, c):
        return linear(linear(a, b), linear(b, c))

    pos = [linear(quadratic(p0[q], p1[q], p2[q]), quadratic(p1[q], p2[q], p3[q])) for q in range(2)]
    u = 1 - t
    tan = [3 * (u * u) * (p1[q] - p0[q]) + 6 * u * t * (p2[q] - p1[q]) + 3 * (t * t) * (p3[q] - p2[q]) for q in range(2)]
    correction = ((target_heading - current_heading) + math.pi) % TWO_PI - math.pi
    heading = current_heading + ((t * correction + math.pi) % TWO_PI - math.pi) - math.pi * 0.5
    return pos[0], pos[1], heading, math.sqrt(tan[0] * tan[0] + tan[1] * tan[1])


def interpolate_trajectory(tr, n, dt):
    """perform_trajectory_interpolation (trajectory_interpolation_provider.py:96-193) on rows time, x, y, heading, speed;
    ``n`` columns given.  Returns (x, y, heading, speed), or None where the reference raises."""
    if n < 2 or n > len(tr[0]):
        return None
    if not all(math.isfinite(float(tr[r][i])) for r in range(5) for i in range(n)):
        return None
    if any(not (tr[0][i] - tr[0][i - 1] > 0) for i in range(1, n)):
        return None
    end = next((i for i in range(n) if tr[0][i] > dt), -1)
    if end < 1:
        return None
    m0, m1 = [float(tr[r][end - 1]) for r in range(5)], [float(tr[r][end]) for r in range(5)]
    ratio = math.fabs((dt - m0[0]) / (m1[0] - m0[0]))
    u = 1 - ratio
    cs = u * math.cos(m0[3]) + ratio * math.cos(m1[3])
    sn = u * math.sin(m0[3]) + ratio * math.sin(m1[3])
    return (u * m0[1] + ratio * m1[1], u * m0[2] + ratio * m1[2], heading_of(math.atan2(sn, cs)), u * m0[4] + ratio * m1[4])


def radians_to_vec(radians):
    angle = (radians + math.pi * 0.5) % TWO_PI
    return math.cos(angle), math.sin(angle)


class BoxChassisRef:
    """BoxChassis (chassis.py:187-320): pose, speed, _last_heading, _last_dt and what the observation reads back."""

    def __init__(self, heading, speed):
        self.heading, self.speed, self.last_heading, self.last_dt = heading, speed, 0.0, 0.0

    def control(self, heading, speed, dt):
        self.last_heading, self.last_dt = self.heading, dt
        self.heading, self.speed = heading, speed

    def read_back(self):
        """speed, linear velocity, angular velocity, yaw rate, steering (NaN = None)."""
        vh = radians_to_vec(self.heading)
        lin = (vh[0] * self.speed, vh[1] * self.speed, 0.0 * self.speed)
        if self.last_dt > 0:
            lh = radians_to_vec(self.last_heading)
            ang = ((vh[0] - lh[0]) / self.last_dt, (vh[1] - lh[1]) / self.last_dt, 0.0)
            yaw_rate = (((self.heading - self.last_heading) + math.pi) % TWO_PI - math.pi) / self.last_dt
        else:
            ang, yaw_rate = (0.0, 0.0, 0.0), math.nan
        return self.speed, lin, ang, yaw_rate, math.nan
