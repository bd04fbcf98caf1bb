"""Inputs of the peak-group tests, shared by tests/test_peakgroup_cpu.py (which measures the tolerance on them with the reference's
variants), tests/test_peakgroup_plan_cpu.py (the planner alone) and tests/test_gpu_peakgroup.py (which runs them on the GPU).  A group
is one cy_fit_peak_groups call: a map, a job table, link and max_iter.  Unless a case says otherwise the starts are the reference's
own single fits (peakfit_ref.fit_peaks), as the chain hands them over.  Blobs are sigma 1.6 x 1.28 px at 30 degrees, R = 6, link 1.5
(entries closer than 9 px are linked); sets of jobs that are not meant to see each other lie more than 24 px apart.
  clean      130 x 170, no noise, pedestal 0.25: pairs 4, 5 and 7 px apart, a chain A~B~C with A not linked to C, a square of four,
             R = 12 beside R = 6 in one group, a pair at the corner (clipped).  The truth of every member is known
  noisy      the same jobs on the same blobs with noise 0.05
  one_iter   `noisy` with max_iter = 1
  edge       130 x 170, noise 0.05: centres exactly Lm apart and one ulp inside; coincident centres; a chain of five (status 7); a
             pair and a hole 3 px from it; a pair beside jobs the planner turns away (status 1 and 5); a pair with an outside
             neighbour 10 px away that takes its share; a hole pair that is the negated copy of a peak pair; NaN, 0 and +-inf
             pixels in a union; two R = 1 discs (status 3); a pair with one inadmissible start (status 4)
  mw403      60 x 403 (MW % 4 != 0): a pair against the right edge
  stage_lo, stage_hi   group windows of 101 x 61 = 6161 (staged in LDS) and 131 x 81 = 10 611 pixels (membership in every sweep)
  random(seed)   peakfit_cases.random(seed) with every job dropped whose centre lies within 3.5 px of an earlier kept job (one blob
             with two "brightest pixels")"""
import math
from types import SimpleNamespace

import numpy as np

import peakfit_cases as PC
import peakfit_ref as PR
import peakgroup_ref as GR
from fit_cases import gauss, truth_params
from peakfit_cases import job, start_of

SIG, RATIO, PA = 1.6, 0.8, 30.0
LINK = 1.5
_CACHE = {}
STATUS_ONLY = ("same_a", "same_b")        # coincident centres: two Gaussians at one place, compared on status and npix only
SEEDS = (1, 2, 3)
GPU_SEED = 3
LEFT_OUT_MAX = PC.LEFT_OUT_MAX
FILTER = 3.5


def with_single_starts(amap, jobs):
    """jobs with the start of every job the reference's single fit ends on (status 0 or 2) replaced by that fit's parameters."""
    jobs = np.array(jobs, np.float64)
    rows = PR.fit_peaks(amap, jobs, 64)
    hit = np.isin(rows[:, 0], (0.0, 2.0))
    jobs[hit, 5:11] = rows[hit, 5:11]
    return jobs


class Scene:
    def __init__(self, MH, MW, noise, seed, pedestal=0.0):
        self.MH, self.MW, self.pedestal = MH, MW, pedestal
        rng = np.random.default_rng(seed)
        self.m = np.full((MH, MW), pedestal) + (rng.normal(0.0, noise, (MH, MW)) if noise else 0.0)
        self.names, self.jobs, self.truth, self.override = [], [], {}, {}

    def blob(self, nm, cx, cy, R=6.0, amp=8.0, sig=SIG, draw=True, sign=1.0, bad=None, **kw):
        if draw:
            self.m = self.m + sign * gauss((self.MH, self.MW), amp, cx + 0.2, cy - 0.1, sig, sig * RATIO, PA)
            self.truth[len(self.jobs)] = truth_params(amp, cx + 0.2, cy - 0.1, sig, sig * RATIO, PA)
        if bad is not None:
            self.override[len(self.jobs)] = bad
        self.names.append(nm)
        self.jobs.append(job(cx, cy, R, start_of(amp, cx, cy, sig), bkg=self.pedestal, sign=sign, **kw))

    def group(self, name, link=LINK, max_iter=64, single=True):
        amap = self.m.astype(np.float32)
        jobs = with_single_starts(amap, self.jobs) if single else np.array(self.jobs, np.float64)
        for e, start in self.override.items():
            jobs[e, 5:11] = start
        return SimpleNamespace(name=name, map=amap, jobs=jobs, names=list(self.names), truth=dict(self.truth), link=link, max_iter=max_iter)


def _layout(s):
    s.blob("pair4_a", 20.0, 20.0); s.blob("pair4_b", 24.0, 20.0, amp=5.0)
    s.blob("pair5_a", 60.0, 20.0); s.blob("pair5_b", 63.0, 24.0, amp=5.0)              # 3-4-5
    s.blob("pair7_a", 100.0, 20.0); s.blob("pair7_b", 107.0, 20.0, amp=5.0)
    s.blob("chain3_a", 20.0, 60.0); s.blob("chain3_b", 27.0, 60.0, amp=6.0); s.blob("chain3_c", 34.0, 60.0, amp=5.0)
    for t, (ox, oy) in enumerate(((0, 0), (6, 0), (0, 6), (6, 6))):
        s.blob("square4_%d" % t, 70.0 + ox, 57.0 + oy, amp=8.0 - t)
    s.blob("r12", 120.0, 60.0, R=12.0, amp=10.0, sig=3.0); s.blob("r6", 130.0, 60.0, amp=6.0)
    s.blob("corner_a", s.MW - 1.0, s.MH - 1.0); s.blob("corner_b", s.MW - 5.0, s.MH - 4.0, amp=5.0)
    return s


CLEAN_PAIRS = (("pair4_a", "pair4_b"), ("pair5_a", "pair5_b"), ("pair7_a", "pair7_b"))
# {name of the group's first member: its members}, the expected structure of `clean` and `noisy`
LAYOUT_GROUPS = {"pair4_a": 2, "pair5_a": 2, "pair7_a": 2, "chain3_a": 3, "square4_0": 4, "r12": 2, "corner_a": 2}


def clean():
    if "clean" not in _CACHE:
        _CACHE["clean"] = _layout(Scene(130, 170, 0.0, 0, pedestal=0.25)).group("clean")
    return _CACHE["clean"]


def noisy():
    if "noisy" not in _CACHE:
        g = _layout(Scene(130, 170, 0.05, 11)).group("noisy")
        g.truth = {}
        _CACHE["noisy"] = g
    return _CACHE["noisy"]


def one_iter():
    g = noisy()
    return SimpleNamespace(name="one_iter", map=g.map, jobs=g.jobs.copy(), names=list(g.names), truth={}, link=g.link, max_iter=1)


def edge():
    if "edge" in _CACHE:
        return _CACHE["edge"]
    s = Scene(130, 170, 0.05, 12)
    s.blob("at_lm_a", 15.0, 15.0); s.blob("at_lm_b", 24.0, 15.0, amp=5.0)                               # exactly 9 = 1.5 * 6: not linked
    s.blob("in_lm_a", 15.0, 45.0); s.blob("in_lm_b", 15.0, math.nextafter(54.0, 0.0), amp=5.0)           # one ulp inside: linked
    s.blob("same_a", 45.0, 15.0); s.blob("same_b", 45.0, 15.0, draw=False)
    for t in range(5):
        s.blob("chain5_%d" % t, 40.0 + 7.0 * t, 45.0, amp=8.0 - t)
    s.blob("hole_pair_a", 95.0, 15.0); s.blob("hole_pair_b", 100.0, 15.0, amp=5.0); s.blob("hole_near", 95.0, 18.0, amp=4.0, sign=-1.0)
    s.blob("away_a", 130.0, 15.0); s.blob("away_b", 135.0, 15.0, amp=5.0)
    s.blob("away_status1", 132.0, 15.0, R=-1.0, draw=False); s.blob("away_status5", 131.5, 15.5, R=0.1, draw=False)
    s.blob("share_a", 100.0, 50.0); s.blob("share_b", 105.0, 50.0, amp=5.0); s.blob("share_out", 115.0, 50.0, amp=6.0)   # 10 px from share_b
    s.blob("invalid_a", 100.0, 85.0); s.blob("invalid_b", 105.0, 85.0, amp=5.0)
    s.blob("r1_a", 140.0, 85.0, R=1.0, sig=0.8); s.blob("r1_b", 141.0, 85.0, R=1.0, draw=False, sig=0.8)
    s.blob("bad_a", 20.0, 115.0); s.blob("bad_b", 25.0, 115.0, amp=5.0, bad=[-1.0, 25.0, 115.0, 0.4, 0.0, 0.4])
    # a peak pair and the hole pair that is its negated copy, 40 columns on
    rng = np.random.default_rng(13)
    patch = gauss((24, 30), 8.0, 12.2, 11.9, SIG, SIG * RATIO, PA) + gauss((24, 30), 5.0, 17.2, 11.9, SIG, SIG * RATIO, PA) + rng.normal(0.0, 0.05, (24, 30))
    patch = patch.astype(np.float32).astype(np.float64)
    s.m[73:97, 8:38], s.m[73:97, 48:78] = patch, -patch
    s.blob("peak_pair_a", 20.0, 85.0, draw=False); s.blob("peak_pair_b", 25.0, 85.0, amp=5.0, draw=False)
    s.blob("neg_pair_a", 60.0, 85.0, draw=False, sign=-1.0); s.blob("neg_pair_b", 65.0, 85.0, amp=5.0, draw=False, sign=-1.0)
    m = s.m
    m[84, 101] = m[87, 104] = np.nan
    m[85, 103] = m[83, 99] = 0.0
    m[86, 100], m[82, 106] = np.inf, -np.inf
    g = s.group("edge")
    g.truth = {}
    _CACHE["edge"] = g
    return g


# what `edge` is about: {job name: (status or None for fitted, nmembers)}
EDGE_EXPECT = {"at_lm_a": (6, 1), "at_lm_b": (6, 1), "in_lm_a": (None, 2), "in_lm_b": (None, 2), "same_a": (None, 2), "chain5_0": (7, 5), "chain5_4": (7, 5),
               "hole_pair_a": (None, 2), "hole_near": (6, 1), "away_a": (None, 2), "away_status1": (1, 0), "away_status5": (5, 0), "share_a": (None, 2),
               "share_out": (6, 1), "invalid_a": (None, 2), "r1_a": (3, 2), "r1_b": (3, 2), "bad_a": (4, 2), "bad_b": (4, 2), "peak_pair_a": (None, 2),
               "neg_pair_a": (None, 2)}


def mw403():
    if "mw403" not in _CACHE:
        s = Scene(60, 403, 0.05, 14)
        s.blob("right_a", 396.0, 30.0); s.blob("right_b", 401.0, 31.0, amp=5.0)
        s.blob("left_a", 3.0, 5.0); s.blob("left_b", 8.0, 4.0, amp=5.0)
        g = s.group("mw403")
        g.truth = {}
        _CACHE["mw403"] = g
    return _CACHE["mw403"]


def staging(R, sep):
    """Two wide blobs `sep` apart with discs of radius R: the group window has (2 R + 1 + sep) x (2 R + 1) pixels."""
    key = "stage%d" % R
    if key not in _CACHE:
        s = Scene(110, 210, 0.05, 15)
        s.blob("wide_a", 60.0, 55.0, R=float(R), amp=40.0, sig=9.0); s.blob("wide_b", 60.0 + sep, 55.0, R=float(R), amp=25.0, sig=8.0)
        g = s.group("stage_lo" if (2 * R + 1 + sep) * (2 * R + 1) <= GR.LDS_MAX else "stage_hi")
        g.truth = {}
        _CACHE[key] = g
    return _CACHE[key]


def stage_lo():
    return staging(30, 40)


def stage_hi():
    return staging(40, 50)


def groups():
    return [clean(), noisy(), one_iter(), edge(), mw403(), stage_lo(), stage_hi()]


def random(seed):
    """peakfit_cases.random(seed) without the jobs within FILTER px of an earlier kept job; the starts are the reference's single fits."""
    key = "random%d" % seed
    if key not in _CACHE:
        g = PC.random(seed)
        keep = []
        for e, j in enumerate(g.jobs):
            if all(math.hypot(j[0] - g.jobs[k, 0], j[1] - g.jobs[k, 1]) > FILTER for k in keep):
                keep.append(e)
        jobs = with_single_starts(g.map, g.jobs[keep])
        _CACHE[key] = SimpleNamespace(name=key, map=g.map, jobs=jobs, names=["j%d" % e for e in keep], truth={}, link=LINK, max_iter=64)
    return _CACHE[key]


def reference(g):
    """The reference's variants on a group, computed once: (list of [n, FIELDS] arrays, the kernel's association first; cond [n])."""
    key = "ref_" + g.name
    if key not in _CACHE:
        _CACHE[key] = GR.fit_variants(g.map, g.jobs, g.link, g.max_iter)
    return _CACHE[key]


def excluded(g):
    res, cond = reference(g)
    return GR.excluded(res, cond)


def group_jobs(res):
    """Boolean [n]: rows of group jobs (status 0, 2, 3 or 4 in the first variant with nmembers >= 2)."""
    return np.isin(res[0][:, 0], (0.0, 2.0, 3.0, 4.0)) & (res[0][:, 6] >= 2)
