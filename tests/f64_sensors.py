"""The projective sensors in float64, restated straight from the reference (no fixtures; shares no code with csrc/, host/ or oracle/):

    perspective_projection          include/mitsuba/render/sensor.h:196-231
    Transform::perspective, look_at include/mitsuba/core/transform.h:203-220, 241-269
    parse_fov                       src/librender/sensor.cpp:113-167
    ThinLensCamera::sample_ray      src/sensors/thinlens.cpp:155-189
    PerspectiveCamera::sample_ray   src/sensors/perspective.cpp:182-216 (no principal point offset)

Matrices are row-major numpy arrays acting on column vectors. The concentric disk map is f64_integrators.disk_concentric."""
import math

import numpy as np

from f64_integrators import disk_concentric


def translate(v):
    m = np.eye(4); m[:3, 3] = v
    return m


def scale(v):
    return np.diag([v[0], v[1], v[2], 1.0])


def perspective(fov, near, far):
    """transform.h:203-220"""
    recip = 1.0 / (far - near)
    cot = 1.0 / math.tan(math.radians(fov * 0.5))
    m = np.diag([cot, cot, far * recip, 0.0])
    m[2, 3] = -near * far * recip
    m[3, 2] = 1.0
    return m


def look_at(origin, target, up):
    """transform.h:241-269 -> camera-to-world"""
    origin, target, up = (np.asarray(a, np.float64) for a in (origin, target, up))
    d = target - origin; d = d / np.linalg.norm(d)
    left = np.cross(up, d); left = left / np.linalg.norm(left)
    new_up = np.cross(d, left)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, new_up, d, origin
    return m


def parse_fov(fov, fov_axis, aspect):
    """sensor.cpp:113-167 for a `fov` property -> the horizontal field of view in degrees"""
    if fov_axis == "smaller":
        fov_axis = "y" if aspect > 1 else "x"
    elif fov_axis == "larger":
        fov_axis = "x" if aspect > 1 else "y"
    if fov_axis == "x":
        return fov
    if fov_axis == "y":
        return math.degrees(2.0 * math.atan(math.tan(0.5 * math.radians(fov)) * aspect))
    if fov_axis == "diagonal":
        diagonal = 2.0 * math.tan(0.5 * math.radians(fov))
        width = diagonal / math.sqrt(1.0 + 1.0 / (aspect * aspect))
        return math.degrees(2.0 * math.atan(width * 0.5))
    raise ValueError(fov_axis)


def perspective_projection(film_size, crop_size, crop_offset, fov_x, near, far):
    """sensor.h:196-231 -> camera_to_sample"""
    fs = np.asarray(film_size, np.float64)
    rel_size = np.asarray(crop_size, np.float64) / fs
    rel_offset = np.asarray(crop_offset, np.float64) / fs
    aspect = fs[0] / fs[1]
    return (scale([1.0 / rel_size[0], 1.0 / rel_size[1], 1.0]) @ translate([-rel_offset[0], -rel_offset[1], 0.0]) @
            scale([-0.5, -0.5 * aspect, 1.0]) @ translate([-1.0, -1.0 / aspect, 0.0]) @ perspective(fov_x, near, far))


class Camera:
    """The state thinlens.cpp:110-146 precomputes, in float64"""

    def __init__(self, film_size, origin, direction, fov=34.0, fov_axis="x", near=1.0, far=35.0, aperture_radius=0.1, focus_distance=None,
                 crop_size=None, crop_offset=(0, 0), up=(0, 1, 0)):
        crop_size = film_size if crop_size is None else crop_size
        self.near, self.far = float(near), float(far)
        self.aperture_radius = float(aperture_radius)
        self.focus_distance = float(far if focus_distance is None else focus_distance)
        self.x_fov = parse_fov(float(fov), fov_axis, film_size[0] / float(film_size[1]))
        origin = np.asarray(origin, np.float64)
        self.to_world = look_at(origin, origin + np.asarray(direction, np.float64), up)
        self.sample_to_camera = np.linalg.inv(perspective_projection(film_size, crop_size, crop_offset, self.x_fov, self.near, self.far))

    def near_p(self, position_sample):
        p = self.sample_to_camera @ np.array([position_sample[0], position_sample[1], 0.0, 1.0])
        return p[:3] / p[3]

    def thinlens_sample_ray(self, position_sample, aperture_sample):
        """thinlens.cpp:166-185 -> (o, d, mint, maxt)"""
        near_p = self.near_p(position_sample)
        tx, ty = disk_concentric((float(aperture_sample[0]), float(aperture_sample[1])))
        aperture_p = np.array([self.aperture_radius * tx, self.aperture_radius * ty, 0.0])
        focus_p = near_p * (self.focus_distance / near_p[2])
        d = focus_p - aperture_p
        d = d / np.linalg.norm(d)
        inv_z = 1.0 / d[2]
        o = self.to_world[:3, :3] @ aperture_p + self.to_world[:3, 3]
        return o, self.to_world[:3, :3] @ d, self.near * inv_z, self.far * inv_z

    def perspective_sample_ray(self, position_sample):
        """perspective.cpp:186-214 -> (o, d, mint, maxt)"""
        d = self.near_p(position_sample)
        d = d / np.linalg.norm(d)
        inv_z = 1.0 / d[2]
        return self.to_world[:3, 3].copy(), self.to_world[:3, :3] @ d, self.near * inv_z, self.far * inv_z
