"""Reference image of the top-down RGB camera (include/smx.h SMX_SENSOR_RGB), composed from the two oracle rasters
the OGM and the DAGM are already held to (oracle/sensors_extra.py): test infrastructure, shared by the RGB tests."""
import math

import numpy as np

from oracle.dynamics import VehicleBody
from oracle.sensors_extra import dagm, ogm
from smarts_amd import _native as nat

# class -> bytes (R, G, B), round(255 * c) of the reference's colours:
#   0  the clear colour (renderer.py:346-395: black)
#   1  SceneColors.Road  = Colors.DarkGrey (colors.py:62 over :47)   (80, 80, 80)
#   2  social vehicles   = Colors.Silver   (colors.py:60 over :33)   (192, 192, 192)
#   3  SceneColors.Agent = Colors.Red      (colors.py:58 over :27)   (210, 30, 30)
PALETTE = np.array([[0, 0, 0], [80, 80, 80], [192, 192, 192], [210, 30, 30]], dtype=np.uint8)


def rgb_ref(ego, agent_bodies, social_bodies, lanes, W, H, res):
    """(H, W, 3) uint8: per pixel the highest class that holds — road, social vehicle, agent vehicle."""
    road = dagm(ego, lanes, W, H, res) == 255
    social = ogm(ego, social_bodies, W, H, res) == 255
    agent = ogm(ego, agent_bodies, W, H, res) == 255
    cls = np.maximum(np.maximum(1 * road, 2 * social), 3 * agent)
    return PALETTE[cls]


def bodies(state, flags):
    """Alive vehicles of ONE env as (agent bodies, social bodies, {slot: body}); `state` = [S_COUNT, N], `flags` = [N]."""
    S = nat.S
    agents, socials, by_slot = [], [], {}
    for j in range(len(flags)):
        if not flags[j] & nat.F_ALIVE:
            continue
        b = VehicleBody(state[S["X"], j], state[S["Y"], j], wrap(float(state[S["HEADING"], j])), 0.0)
        (socials if flags[j] & nat.F_SOCIAL else agents).append(b)
        by_slot[j] = b
    return agents, socials, by_slot


def wrap(h):
    """wrap_heading of the device code (smx_device.h): a state row may hold a heading outside (-pi, pi]."""
    v = h % (2 * math.pi)
    return v - 2 * math.pi if v > math.pi else v
