"""The described source, restated in numpy (include/neutral_hip.h: neutral_hip_source_described).

    refilled          the fixed source's slots (source_reference.ranks): the first count dead ones
    C_k, S            the running sums of the components' shares, S the last; B_{k,b}, S_k those of
                      component k's bins (np.cumsum: one addition each, left to right)
    slot j            counter 2 of the stream (pkey = pid_base + j, master_key = seed) chooses:
                      t = u0 * S, the first k with t < C_k, else the last; tb = u1 * S_k, the first
                      of k's bins with tb < B_{k,b}, else its last.  Counter 0 places it in k's box,
                      counter 1 gives theta = theta0 + theta_width * d0 and the energy
                      e_lo + d1 * (e_hi - e_lo), e_lo itself for a line; weight, dt,
                      mfp_to_collision 0, dead 0 as the fixed source has them

A description is a list of components (share, box, bins, theta): box = (left, bottom, width,
height), bins = [(e_lo, e_hi, share), ...], theta = (theta0, theta_width).  The samples of the
streams are an input (`rn`, shape (slots, 3, 2): counters 0, 1, 2): on the GPU they come from the
library's own Threefry (probe_rows and interface.probe_threefry), on the CPU from the oracle's
(cpu_samples).  The choices are single multiplications and comparisons, the same bits everywhere;
positions, angles and bin energies agree with the device's to a rounding, not to the bit.
"""
from collections import namedtuple

import numpy as np

import source_reference as sr

F64_FIELDS, I32_FIELDS, FIELDS = sr.F64_FIELDS, sr.I32_FIELDS, sr.FIELDS

Component = namedtuple("Component", "share box bins theta")
ISOTROPIC = (0.0, 2.0 * np.pi)

# the block's offsets in the mesh, dt, the block's edge arrays (pad removed)
MeshArgs = namedtuple("MeshArgs", "x_off y_off dt edgex edgey")


def component(share, box, energies, theta=ISOTROPIC) -> Component:
    """energies: (e, share) lines and (e_lo, e_hi, share) bins, as interface.SourceComponent takes them"""
    bins = [(e[0], e[0], e[1]) if len(e) == 2 else tuple(e) for e in energies]
    return Component(float(share), tuple(float(v) for v in box), [tuple(float(v) for v in b) for b in bins],
                     tuple(float(v) for v in theta))


def degenerate(args: sr.SourceArgs):
    """the description that is the fixed source of `args`: its box, every direction, one line"""
    return [component(1.0, (args.left, args.bottom, args.width, args.height), [(args.energy, 1.0)])]


def mesh_of(args: sr.SourceArgs) -> MeshArgs:
    return MeshArgs(args.x_off, args.y_off, args.dt, args.edgex, args.edgey)


def to_interface(iface, description):
    """the same description as an interface.SourceDescription"""
    return iface.SourceDescription([iface.SourceComponent(c.share, c.box, c.bins, c.theta) for c in description])


def probe_rows(slots, pid_base: int, seed: int) -> np.ndarray:
    """rows {counter, pkey, master_key} for interface.probe_threefry: counters 0, 1 and 2 of every
    slot; its samples reshaped (-1, 3, 2) are `rn`"""
    slots = np.asarray(slots, dtype=np.uint64)
    rows = np.empty((len(slots), 3, 3), dtype=np.uint64)
    rows[:, 0, 0], rows[:, 1, 0], rows[:, 2, 0] = 0, 1, 2
    rows[:, :, 1] = (np.uint64(pid_base) + slots)[:, None]
    rows[:, :, 2] = np.uint64(seed)
    return rows.reshape(-1, 3)


def cpu_samples(slots, pid_base: int, seed: int) -> np.ndarray:
    """rn[i, counter] = the two samples of slot i's stream at that counter, from the oracle's Threefry"""
    import oracle_binding as ob
    rn = np.empty((len(slots), 3, 2), dtype=np.float64)
    for i, j in enumerate(slots):
        for counter in (0, 1, 2):
            rn[i, counter] = ob.generate_random_numbers(int(pid_base) + int(j), int(seed), counter)
    return rn


def first_below(t: np.ndarray, cumulative: np.ndarray) -> np.ndarray:
    """per element of t: the first index i with t < cumulative[i], else the last index"""
    below = t[:, None] < cumulative[None, :]
    return np.where(below.any(axis=1), below.argmax(axis=1), len(cumulative) - 1)


def choose(description, u):
    """(component, bin within the component) of every slot from counter 2's samples u[:, 0:2]"""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 2)
    c_cum = np.cumsum(np.array([c.share for c in description], dtype=np.float64))
    k = first_below(u[:, 0] * c_cum[-1], c_cum)
    b = np.zeros(len(u), dtype=np.int64)
    for i, c in enumerate(description):
        b_cum = np.cumsum(np.array([s for _, _, s in c.bins], dtype=np.float64))
        mine = k == i
        b[mine] = first_below(u[mine, 1] * b_cum[-1], b_cum)
    return k, b


def expected(before: dict, dead, count: int, weight: float, seed: int, pid_base: int, description,
             mesh: MeshArgs, rn=None):
    """-> (the arrays after the call (new arrays), the component of every refilled slot, its bin);
    rn: see the module's text (None: the oracle's)"""
    slots = sr.ranks(dead, count)
    if rn is None:
        rn = cpu_samples(slots, pid_base, seed)
    rn = np.asarray(rn, dtype=np.float64).reshape(len(slots), 3, 2)
    k, b = choose(description, rn[:, 2])
    box = np.array([c.box for c in description], dtype=np.float64).reshape(-1, 4)[k]
    theta = np.array([c.theta for c in description], dtype=np.float64).reshape(-1, 2)[k]
    bins = np.array([description[ki].bins[bi][:2] for ki, bi in zip(k, b)], dtype=np.float64).reshape(-1, 2)
    out = {f: np.array(before[f]) for f in FIELDS}
    x = box[:, 0] + rn[:, 0, 0] * box[:, 2]
    y = box[:, 1] + rn[:, 0, 1] * box[:, 3]
    angle = theta[:, 0] + theta[:, 1] * rn[:, 1, 0]
    e_lo, e_hi = bins[:, 0], bins[:, 1]
    out["x"][slots], out["y"][slots] = x, y
    out["cellx"][slots] = mesh.x_off + sr.find_cell(mesh.edgex, x)
    out["celly"][slots] = mesh.y_off + sr.find_cell(mesh.edgey, y)
    out["omega_x"][slots], out["omega_y"][slots] = np.cos(angle), np.sin(angle)
    out["energy"][slots] = np.where(e_hi == e_lo, e_lo, e_lo + rn[:, 1, 1] * (e_hi - e_lo))
    out["weight"][slots] = weight
    out["dt_to_census"][slots] = mesh.dt
    out["mfp_to_collision"][slots] = 0.0
    out["dead"][slots] = 0
    return out, k, b
