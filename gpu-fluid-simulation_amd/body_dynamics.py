"""A dynamic body on the host, 2D or 3D: the loads the engine reports (include/fluidsim.h "2D body loads"; "3D
body loads", §26) integrated into the pose that set_body_motion takes.  The engine's bodies stay kinematic; this closes the loop
outside it."""
import numpy as np


class BodyDynamics2D:
    """Mass, moment of inertia, gravity and the state (centre, angle, velocity, angular velocity) of one body, in float64.
    `particle_mass`: the mass one fluid particle stands for, which turns the engine's per-unit-mass sums into momentum.
    `lock_x`, `lock_y`, `lock_rotation` hold a degree of freedom fixed: both axes locked is a hinge (torque only), one axis and the
    rotation locked a slider."""

    def __init__(self, mass, inertia, centre, angle=0.0, velocity=(0.0, 0.0), angular_velocity=0.0, gravity=(0.0, 0.0),
                 particle_mass=1.0, lock_x=False, lock_y=False, lock_rotation=False):
        if not (mass > 0.0 and inertia > 0.0):
            raise ValueError("BodyDynamics2D: mass and inertia must be > 0")
        self.mass, self.inertia, self.particle_mass = float(mass), float(inertia), float(particle_mass)
        self.centre = np.array(centre, dtype=np.float64)
        self.velocity = np.array(velocity, dtype=np.float64)
        self.gravity = np.array(gravity, dtype=np.float64)
        self.angle, self.angular_velocity = float(angle), float(angular_velocity)
        self.free = np.array([not lock_x, not lock_y], dtype=bool)
        self.free_rotation = not lock_rotation

    def integrate(self, impulse, angular_impulse, dt):
        """One semi-implicit Euler step from the momentum (float64 [2]) and the angular momentum the fluid handed over during the
        last step: the velocities first, the pose from the NEW velocities.  A locked degree of freedom keeps its velocity."""
        dt = float(dt)
        dv = np.asarray(impulse, dtype=np.float64) / self.mass + self.gravity * dt
        self.velocity = np.where(self.free, self.velocity + dv, self.velocity)
        if self.free_rotation:
            self.angular_velocity += float(angular_impulse) / self.inertia
        self.centre = self.centre + self.velocity * dt
        self.angle += self.angular_velocity * dt

    def motion(self):
        """(centre float32 [2], rot float32 [4], velocity float32 [2], angular_velocity): set_body_motion's arguments after the
        slot; the rotation in rigid_motion2d's convention (row-major R, world = R * local, counter-clockwise by `angle`)."""
        c, s = np.cos(self.angle), np.sin(self.angle)
        rot = np.array([c, -s, s, c], dtype=np.float64).astype(np.float32)
        return self.centre.astype(np.float32), rot, self.velocity.astype(np.float32), np.float32(self.angular_velocity)

    def advance(self, sim, slot, tick):
        """Between two steps: reads and resets the slot's loads — ONE SYNC PER STEP, the price of integrating on the host —
        integrates over tick.delta and sets the body's motion for the next step.  Returns the BodyLoads it read."""
        loads = sim.body_loads(slot, reset=True)
        self.integrate(loads.impulse(self.particle_mass), loads.angular_impulse(self.particle_mass), tick.delta)
        sim.set_body_motion(slot, *self.motion())
        return loads


class BodyDynamics3D:
    """Mass, principal moments of inertia (Ix, Iy, Iz) in the body frame, gravity and the state of one 3D body in float64: centre,
    rotation matrix R in rigid_motion's convention (world = R * local), velocity and the angular momentum L in the world frame.
    `particle_mass`: the mass one fluid particle stands for.  `lock_x`, `lock_y`, `lock_z` and `lock_rotation` hold a degree of
    freedom fixed: a locked axis keeps its velocity, a locked rotation keeps L."""

    def __init__(self, mass, inertia, centre, rot=None, velocity=(0.0, 0.0, 0.0), angular_momentum=(0.0, 0.0, 0.0),
                 gravity=(0.0, 0.0, 0.0), particle_mass=1.0, lock_x=False, lock_y=False, lock_z=False, lock_rotation=False):
        self.inertia = np.array(inertia, dtype=np.float64).reshape(3)
        if not (mass > 0.0 and (self.inertia > 0.0).all()):
            raise ValueError("BodyDynamics3D: mass and the three moments of inertia must be > 0")
        self.mass, self.particle_mass = float(mass), float(particle_mass)
        self.centre = np.array(centre, dtype=np.float64).reshape(3)
        self.rot = np.eye(3) if rot is None else np.array(rot, dtype=np.float64).reshape(3, 3)
        self.velocity = np.array(velocity, dtype=np.float64).reshape(3)
        self.angular_momentum = np.array(angular_momentum, dtype=np.float64).reshape(3)
        self.gravity = np.array(gravity, dtype=np.float64).reshape(3)
        self.free = np.array([not lock_x, not lock_y, not lock_z], dtype=bool)
        self.free_rotation = not lock_rotation

    @property
    def angular_velocity(self):
        """w = R diag(1/I) R^T L, world frame, float64 [3]"""
        return self.rot @ ((self.rot.T @ self.angular_momentum) / self.inertia)

    def integrate(self, impulse, angular_impulse, dt):
        """One semi-implicit Euler step from the momentum and the angular momentum (float64 [3] each) the fluid handed over during
        the last step: v and L first, the pose from the NEW v and w.  R is turned by the rotation of angle |w| dt about w / |w|
        (Rodrigues' formula; |w| = 0: unchanged)."""
        dt = float(dt)
        dv = np.asarray(impulse, dtype=np.float64) / self.mass + self.gravity * dt
        self.velocity = np.where(self.free, self.velocity + dv, self.velocity)
        if self.free_rotation:
            self.angular_momentum = self.angular_momentum + np.asarray(angular_impulse, dtype=np.float64)
        self.centre = self.centre + self.velocity * dt
        w = self.angular_velocity
        rate = float(np.sqrt((w * w).sum()))
        if rate > 0.0:
            a, th = w / rate, rate * dt
            kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
            self.rot = (np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)) @ self.rot

    def motion(self):
        """(centre float32 [3], rot float32 [9], velocity float32 [3], angular_velocity float32 [3]): FluidSimulation3D.
        set_body_motion's arguments after the slot."""
        return (self.centre.astype(np.float32), self.rot.astype(np.float32).reshape(9), self.velocity.astype(np.float32),
                self.angular_velocity.astype(np.float32))

    def advance(self, sim, slot, tick):
        """Between two steps: reads and resets the slot's loads — ONE SYNC PER STEP, the price of integrating on the host —
        integrates over tick.delta and sets the body's motion for the next step.  Returns the BodyLoads3D it read."""
        loads = sim.body_loads(slot, reset=True)
        self.integrate(loads.impulse(self.particle_mass), loads.angular_impulse(self.particle_mass), tick.delta)
        sim.set_body_motion(slot, *self.motion())
        return loads
