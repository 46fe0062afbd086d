"""One resolution level of a pairwise discrete registration, as the reference's callers drive the hot path:

    Mesh_registration::run_discrete_opt                 M/mesh_registration.cpp:164-232
    NonLinearSRegDiscreteModel::Initialize              M/DiscreteModel.cpp:63-108
    NonLinearSRegDiscreteModel::setupCostFunction       M/DiscreteModel.cpp:216-262
    NonLinearSRegDiscreteModel::applyLabeling           M/DiscreteModel.cpp:264-269
    MCMC::optimise                                      M/mcmc_opt.h:31-134   (the optimiser without a licence restriction)

The loop itself is caller logic; everything it calls goes through an `ops` object.  `ProductOps` (below) maps the calls to
libmsmhip through the C ABI; the parity tests pass an oracle-backed object with the same methods, so that the two runs
differ in nothing but the implementation of the path (tests/helpers.py, tests/test_gpu_registration.py).
"""
import sys
import threading
import time

import numpy as np

from . import api

RAD = 100.0  # M/reg_tools.h
EXCL_WITH_WEIGHTINGS = ("--excl together with --inweight and --refweight is not available: downsample_cfweighting (M/mesh_registration.cpp:334-350) reads the "
                        "level grid's exclusion mask at vertex numbers of the weightings' own meshes, which is out of bounds or meaningless unless the two "
                        "meshes have the same size")


def _mplp_host(unary, tcosts, triplets, labeling, sweeps, forbid=False):
    """the MPLP branch of run_discrete_level over fetched tables: the host literal's labelling (any ops without an mplp method of its own gets this)"""
    return api.mplp_optimise(unary, tcosts, triplets, labeling, sweeps=sweeps, bound=False, forbid=forbid).labeling


def _mplp_round_host(unary, tcosts, triplets, labeling, sweeps, polish, forbid=False):
    """the same with the rounding (DESIGN.md 5.19 "Rounding"): the sweeps, mode 0 on their messages with their winner handed in, one mode-1 call on the
    result -- what msm_cost_mplp_round(then_polish) does over the device tables"""
    r = api.mplp_optimise(unary, tcosts, triplets, labeling, sweeps=sweeps, bound=False, messages=True, forbid=forbid)
    lab = api.mplp_round(unary, tcosts, triplets, r.labeling, messages=r.messages, mode=0, polish=polish, forbid=forbid).labeling
    return api.mplp_round(unary, tcosts, triplets, lab, mode=1, polish=polish, forbid=forbid).labeling


def _mplp_pairs_host(unary, paircosts, pairs, labeling, sweeps, polish=0):
    """the pairwise MPLP branch of run_discrete_level over fetched tables: the host literal's labelling, polished where polish > 0 -- what
    msm_cost_mplp_pairs_optimise does over the device tables"""
    lab = api.mplp_pairs_optimise(unary, paircosts, pairs, labeling, sweeps=sweeps, bound=False).labeling
    return api.mplp_pairs_polish(unary, paircosts, pairs, lab, polish=polish).labeling if polish > 0 else lab


class ProductOps:
    """The calls of the level loop on the MI355X path (every method is one or two C-ABI calls)."""

    def __init__(self, ctx, mcmc_gpu=False, features_gpu=False, mcmc_draw_gpu=False, mplp_gpu=True, mplp_round=False, mplp_polish=8,
                 mplp_forbid=False, mplp_pairs=False, fusion_mplp=False, fusion_sweeps=10, fusion_polish=8):
        """features_gpu: the level loops prepare a level's features for all data sets through ONE call (level_features_batch: msm_level_features, with
        the masked list surgery and create_exclusion on the device) instead of the chain of calls of level_features / finish_features -- the same
        bytes (what MSMHIP_FEATURES=gpu asks of the executables).
        mcmc_gpu: the MCMC branch of run_discrete_level leaves both tables on the device and runs the sweeps there (msm_cost_mcmc_optimise) instead
        of fetching them for the host optimiser -- the same labelings, bit for bit (what MSMHIP_MCMC=gpu asks of the executables).
        mcmc_draw_gpu (with mcmc_gpu): those sweeps take their proposals from the draw kernel instead of the host's stream (the context's
        set_mcmc_draw) -- the same proposals, bit for bit (what MSMHIP_MCMC_DRAW=gpu asks of the executables)
        mplp_gpu: the MPLP branch of run_discrete_level (optimiser="mplp", an extension) leaves both tables on the device and runs its sweeps there
        (msm_cost_mplp_optimise); False fetches them for the host literal (msm_mplp_optimise) -- the same labelings, bit for bit
        mplp_round: an iteration of the MPLP branch rounds the final messages to a labelling after its sweeps (the conditioned decode and mplp_polish
        polish passes, then one polish call on the winner: msm_cost_mplp_round, or msm_mplp_round over the fetched tables -- the same labelings; what
        MSMHIP_MPLP_ROUND=on and MSMHIP_MPLP_POLISH=n ask of the executables)
        mplp_forbid: the MPLP branch reads NaN and +inf entries of the triplet table as forbidden label combinations instead of refusing the table
        (DESIGN.md 5.19 "Forbidden entries"; the strain regulariser produces them wherever a label set lets control points meet), on the device route
        (msm_cost_set_mplp_forbid) and on the host route (msm_mplp_optimise_forbid) alike; what MSMHIP_MPLP_FORBID=on asks of the executables
        mplp_pairs: what MSMHIP_MPLP_PAIRS=on asks of the executables -- --dopt=MPLP with --regoption=1 runs as optimiser "mplp_pairs" (MPLP over the
        unary and pair tables; config.levels_from_config(mplp_pairs=True) names it), and run_discrete_level refuses that optimiser without it.  That branch follows mplp_gpu (tables and sweeps on
        the device: msm_cost_mplp_pairs_optimise) and, with mplp_round, polishes the sweeps' winner with mplp_polish passes; it ignores mplp_forbid
        fusion_mplp: the binary problem of every label step of run_discrete_level(optimiser="fusion") is solved by MPLP (an extension, DESIGN.md 5.21:
        fusion_sweeps sweeps from x = 0, then the rounding with fusion_polish polish passes) instead of the stand-in fusion_step -- with mplp_gpu in one
        launch behind the step's own kernel (msm_cost_fusion_mplp_step), without it by the host literal over the fetched octets
        (msm_fusion_mplp_step): the same labellings; what MSMHIP_FUSION=mplp, MSMHIP_FUSION_SWEEPS=n and MSMHIP_FUSION_POLISH=n ask of the executables.
        Groupwise label steps (pair factors) keep the stand-in."""
        self.ctx = ctx
        self.fusion_mplp = bool(fusion_mplp)
        self.fusion_sweeps, self.fusion_polish = int(fusion_sweeps), int(fusion_polish)
        if not 1 <= self.fusion_sweeps <= 256:
            raise ValueError("fusion_sweeps: the sweeps of a label step's MPLP solve are a whole number from 1 to 256")
        if not 0 <= self.fusion_polish <= 64:
            raise ValueError("fusion_polish: the polish passes of a label step's MPLP solve are a whole number from 0 to 64")
        self.mplp_forbid = bool(mplp_forbid)
        self.mplp_pairs = bool(mplp_pairs)
        self.mplp_round = bool(mplp_round)
        self.mplp_polish = int(mplp_polish)
        if not 0 <= self.mplp_polish <= 64:
            raise ValueError("mplp_polish: the polish passes of the rounding are a whole number from 0 to 64")
        self.mplp_gpu = bool(mplp_gpu)
        self.mcmc_gpu = bool(mcmc_gpu)
        self.mcmc_draw_gpu = bool(mcmc_draw_gpu)
        if self.mcmc_draw_gpu:
            if not self.mcmc_gpu:
                raise ValueError("mcmc_draw_gpu draws the proposals of the GPU sweeps: it needs mcmc_gpu")
            ctx.set_mcmc_draw(1)
        self.features_gpu = bool(features_gpu)

    # --- meshes
    def icosphere(self, order):
        return api.make_mesh_from_icosa(order)

    def mesh(self, xyz, tri, feat=None):
        m = api.Mesh(self.ctx, xyz, tri)
        if feat is not None:
            m.set_pvalues(feat)
        return m

    def set_coords(self, mesh, xyz):
        mesh.set_coords(xyz)

    def coords(self, mesh):
        return mesh.get_coords()

    def unfold(self, mesh):
        return mesh.unfold(RAD)

    def sphere_project_warp(self, sphere_xyz, from_mesh, to_xyz):
        return api.sphere_project_warp(sphere_xyz, from_mesh, to_xyz)

    def warp_mesh(self, mesh, from_mesh, to_xyz):
        """sphere_project_warp of the coordinates `mesh` holds, in place (on the device: no host round trip of the 3 x V arrays)"""
        api.sphere_project_warp_mesh(mesh, from_mesh, to_xyz)

    # --- featurespace::initialise
    def metric_resample(self, in_mesh, data, new_mesh, slot=None, excl=None):
        """slot (optional): a name under which the result may live in a pinned buffer of the context that the NEXT call with the same name reuses
        (the copy engine writes it directly: no staging memcpy of the D x V matrix); None: a fresh numpy array.  excl (optional, V(in_mesh): the
        --excl mask, 0 = excluded): returns (data, the resampled mask), both fresh arrays"""
        if excl is not None:
            return api.metric_resample(in_mesh, data, new_mesh, excl=excl)
        if slot is None:
            return api.metric_resample(in_mesh, data, new_mesh)
        out = self.ctx.scratch_host_array("metric_resample:" + slot, (np.atleast_2d(data).shape[0], new_mesh.V))
        return api.metric_resample(in_mesh, data, new_mesh, out=out)

    def pin(self, array):
        """a large input matrix in page-locked memory of the context for the length of a run (msm_host_alloc: one copy here, and every level's upload of
        it then skips the staging blocks).  Returns (token for unpin, the array to use); (None, array) when the array is small or not float64.
        (Until round 5 the caller's own numpy array was page-locked in place (msm_host_register).  Page-locking works on whole pages and the device address
        of such memory is its host address: the first and last page of an array in the heap are shared with its heap neighbours, and the HIP runtime
        page-locks and releases pageable buffers of asynchronous copies on its own -- whichever of two sharers is released first unmaps the page under the
        other.  msm_host_register now refuses ranges that are not whole pages)"""
        a = np.asarray(array)
        if a.dtype != np.float64 or a.nbytes < (1 << 20):
            return None, array
        try:
            pinned = self.ctx.host_array(a.shape)
        except api.MsmError:
            return None, array
        pinned[...] = a
        return pinned, pinned

    def unpin(self, token):
        if token is not None:
            self.ctx.release_host_array(token)

    def smooth_data(self, mesh, data, sigma, excl=None):
        """with excl (V(mesh)): returns (data, the smoothed mask)"""
        return api.smooth_data(mesh, data, mesh, sigma, excl=excl)

    def variance_normalise(self, data, excl=None):
        return api.variance_normalise(data, excl=excl)

    def create_exclusion(self, data, thrl, thru):
        return api.create_exclusion(data, thrl, thru)

    def histogram_match(self, srcs, ref, src_excls=None, ref_excl=None):
        """multivariate_histogram_normalization (--IN / --INc) of every matrix of the list `srcs` (equal shapes) against the one target `ref`, with
        their masks (a list like srcs, and the target's; both or none): ONE call, the target's statistics are computed once.  Returns the list of
        matched copies."""
        out = api.histogram_match(self.ctx, np.stack([np.atleast_2d(s) for s in srcs]), ref, None if src_excls is None else np.stack(src_excls), ref_excl)
        return list(out)

    def level_features_batch(self, ico, meshes, datas, sigmas, exclude, intensity, varnorm, cutthr):
        """featurespace::initialise for the data sets (meshes[i], datas[i]) on the level grid ico in one call (msm_level_features): what
        composed_level_features gives over this object's other methods.  Returns (list of D x V(ico) features, list of masks -- None each without exclude)"""
        feat, mask = api.level_features(ico, meshes, datas, sigmas, exclude=exclude, intensity=intensity, varnorm=varnorm, cutthr=cutthr)
        return list(feat), ([None] * len(meshes) if mask is None else list(mask))

    def nearest_neighbour(self, mesh, data, q_xyz):
        return api.nearest_neighbour_interpolation(mesh, data, q_xyz)

    # --- aMSM (--regoption=5): Mesh_registration::resample_anatomy, M/mesh_registration.cpp:250-332
    def resample_anatomy_grid(self, cp_xyz, cp_tri, levels):
        return api.resample_anatomy_grid(cp_xyz, cp_tri, levels, RAD)

    def surface_resample(self, anat_xyz, sphere_mesh, q_xyz):
        """newresampler::surface_resample / project_anatomical_mesh (R/resampler.cpp:284-302, :260-282): the anatomy given on the vertices of sphere_mesh at q"""
        return api.barycentric_coords_resample(sphere_mesh, anat_xyz, q_xyz)

    # --- model host logic
    def cp_spacings(self, mesh, xyz, tri):
        return api.cp_spacings(xyz, tri)

    def estimate_triplets(self, mesh, tri):
        return api.estimate_triplets(tri)

    def estimate_pairs(self, mesh, tri, nodes):
        return api.estimate_pairs(tri, nodes)

    def label_sampling_grid(self, sg_order, max_dist):
        return api.label_sampling_grid(sg_order, max_dist)

    def rescale_sampling_grid(self, samples, scale):
        return api.rescale_sampling_grid(samples, scale)

    def cp_rotations(self, centre, cp_xyz):
        return api.cp_rotations(centre, cp_xyz)

    # --- cost function
    def cost(self, kind, simmeasure, rmode, params, target, source, cpgrid, src_feat):
        cf = api.DiscreteCostFunction(self.ctx, kind=kind, simmeasure=simmeasure, rmode=rmode, **params)
        cf.set_meshes(target, source, cpgrid)
        cf.set_featurespace(src_feat)
        if self.mplp_forbid:
            cf.set_mplp_forbid(True)
        return _ProductCost(cf)

    def mcmc(self, unary, tcosts, triplets, labeling, mcparam, iters, seed):
        return api.mcmc_optimise(unary, tcosts, triplets, labeling, mcparam=mcparam, iters=iters, seed=seed)

    def mcmc_chains(self, unary, tcosts, triplets, labeling, mcparam, iters, seeds):
        return api.mcmc_optimise_chains(unary, tcosts, triplets, labeling, seeds, mcparam=mcparam, iters=iters)[0]

    def mplp(self, unary, tcosts, triplets, labeling, sweeps):
        if self.mplp_round:
            return _mplp_round_host(unary, tcosts, triplets, labeling, sweeps, self.mplp_polish, self.mplp_forbid)
        return _mplp_host(unary, tcosts, triplets, labeling, sweeps, self.mplp_forbid)

    def mplp_pairs_solve(self, unary, paircosts, pairs, labeling, sweeps):
        return _mplp_pairs_host(unary, paircosts, pairs, labeling, sweeps, self.mplp_polish if self.mplp_round else 0)

    def fusion_mplp_step(self, unary2, octets, triplets):
        """the label step's binary problem by the host literal of DESIGN.md 5.21: api.FusionMplp"""
        return api.fusion_mplp_step(unary2, octets, triplets, sweeps=self.fusion_sweeps, polish=self.fusion_polish)

    def fusion_step(self, unary2, octets, triplets, passes, quads=None, pairs=None):
        return api.fusion_icm_step(unary2, octets, triplets, passes, quads=quads, pairs=pairs)

    def pairwise_solve(self, unary, paircosts, pairs, passes):
        return api.pairwise_icm(unary, paircosts, pairs, passes=passes)

    # --- rigid level
    def rigid_level(self, target_xyz, target_tri, ref_feat, source_xyz, source_tri, src_feat, sph_in, iters, simmeasure, stepsize, gradsampling):
        """Rigid_cost_function(SPH_orig, SPH_orig, FEAT) + initialise, update_source(sph_in), run (M/mesh_registration.cpp:66-72, 112-116):
        returns (the rotated data grid, the optimiser's trace)"""
        target = self.mesh(target_xyz, target_tri)
        source = target if source_xyz is target_xyz else self.mesh(source_xyz, source_tri)
        rcf = api.RigidCostFunction(self.ctx, target, source, src_feat, ref_feat, simmeasure=simmeasure).initialise()
        try:
            rcf.update_source(sph_in)
            xyz, trace, _ = rcf.run(iters=iters, stepsize=stepsize, gradsampling=gradsampling)
        finally:
            rcf.close()
        return xyz, trace


class _ProductCost:
    def __init__(self, cf):
        self.cf = cf
        self._octets = None

    def reset_source(self, mesh):
        self.cf.reset_source(mesh)

    def reset_cpgrid(self, mesh):
        self.cf.reset_CPgrid(mesh)

    def set_spacings(self, maxsep, mvdmax):
        self.cf.set_spacings(maxsep, mvdmax)

    def set_cfweight(self, w):
        self.cf.set_dataaffintyweighting(w)

    def set_labels(self, labels, rot):
        self.cf.set_labels(labels, rot)

    def set_triplets(self, triplets):
        self.cf.setTriplets(triplets)

    def set_pairs(self, pairs):
        self.cf.setPairs(pairs)

    def set_anatomical(self, sphere_mesh, atarget_xyz, asource_xyz, grid):
        self.cf.set_anatomical(sphere_mesh, atarget_xyz, asource_xyz, grid["sphere_tri"], grid["w_ptr"], grid["w_cp"], grid["w_val"], grid["face_ptr"],
                               grid["face_idx"])

    def get_source_data(self):
        self.cf.get_source_data()

    def unary_table(self):
        return self.cf.computeUnaryCosts()

    def pairwise_table(self):
        return self.cf.computePairwiseCosts()

    def triplet_table(self):
        return self.cf.computeTripletCosts(pinned=True)  # consumed by the optimiser before the next table is computed

    def _octet_buffers(self):
        # the optimiser's per-step buffers: mapped pinned memory the kernel writes (two grow-only buffers per context, used in turn: a step's costs are
        # consumed by its solve while the next step may already be written into the other); the numpy views are made once per set of triplets
        if self._octets is None or self._octets[0].shape[0] != self.cf.T:
            self._octets = [self.cf.ctx.scratch_host_array("octets%d" % k, (self.cf.T, 8)) for k in range(2)]
            self._turn = 0
        return self._octets

    def triplet_octets(self, labeling, label):
        bufs = self._octet_buffers()
        out = bufs[self._turn]
        self._turn ^= 1
        return self.cf.tripletOctets(labeling, label, out)

    def prefetch_octets(self, labeling, label):
        """the NEXT triplet_octets call will ask for (labeling, label) unless the solve in between changes a label: let its kernel run meanwhile
        (msm_cost_triplet_octets_prefetch into the buffer that call will use)"""
        self.cf.prefetchTripletOctets(labeling, label, self._octet_buffers()[self._turn])

    def mcmc_optimise(self, labeling, mcparam, iters, seed):
        return self.cf.mcmc_optimise(labeling, mcparam=mcparam, iters=iters, seed=seed)

    def mcmc_optimise_chains(self, labeling, mcparam, iters, seeds):
        return self.cf.mcmc_optimise_chains(labeling, seeds, mcparam=mcparam, iters=iters)[0]

    def mplp_optimise(self, labeling, sweeps):
        return self.cf.mplp_optimise(labeling, sweeps=sweeps, bound=False).labeling

    def mplp_round(self, labeling, sweeps, polish):
        return self.cf.mplp_round(labeling, sweeps=sweeps, polish=polish, then_polish=True)[0].labeling

    def fusion_mplp_step(self, labeling, label, sweeps, polish):
        return self.cf.fusion_mplp_step(labeling, label, sweeps=sweeps, polish=polish)

    def mplp_pairs_optimise(self, labeling, sweeps, polish):
        return self.cf.mplp_pairs_optimise(labeling, sweeps=sweeps, polish=polish, bound=False)[0].labeling

    def total(self, labeling):
        return self.cf.evaluateTotalCostSum(labeling)[0]


def hcp_msmall_levels(iterations=(10, 15, 15)):
    """The schedule of config/HCP_multimodal_alignment/MSMAllStrainFinalconf1to1_1to3_2 (BASELINE config 3) for run_multiresolution, read from
    the configuration text itself (newmsm_amd/config.py: PRESETS["HCP_MSMAll"] through the reference's grammar, float options rounded to
    float32 as the reference's option parser does): --CPgrid=2,3,4 --datagrid=4,5,6 --SGgrid=4,5,6 --it=10,15,15 --lambda=0.00001,0.0075,0.01
    --regoption=3 --regexp=2 --k_exponent=2 --bulkmod=1.6 --shearmod=0.4 --sigma_in/ref=0 --simval=2, with --triclique (the HO classes over
    the 32 feature rows of the MSMAll data), --rescaleL, --VN (pass varnorm=True) and --dopt=HOCR (optimiser "fusion": the label loop of
    Fusion::optimize; its binary solve is a stand-in, see run_discrete_level)."""
    from . import config

    return config.preset_levels("HCP_MSMAll", 32, iterations)[0]


def basic_levels(iterations=(3, 3, 3)):
    """Three DISCRETE levels shaped like config/basic_configs/config_standard_MSM_strain (--CPgrid=2,3,4 --datagrid=4,5,6 --SGgrid=4,5,6,
    --sigma_in/ref=4,2,1, pass varnorm=True for its --VN); optimiser, cost class and regulariser come from the caller's keyword arguments."""
    return [dict(data_order=4 + k, cp_order=2 + k, sigma_in=s, sigma_ref=s, iters=iterations[k]) for k, s in enumerate((4.0, 2.0, 1.0))]


def apply_labeling(rot, labels, labeling):
    """m_CPgrid.set_coord(i, m_ROT[i] * m_labels[labeling[i]]), operator*(Matrix, Point) R/point.cpp:207-213 (row sums left to right)"""
    R = np.asarray(rot).reshape(-1, 3, 3)
    v = np.asarray(labels)[np.asarray(labeling)]
    return R[:, :, 0] * v[:, None, 0] + R[:, :, 1] * v[:, None, 1] + R[:, :, 2] * v[:, None, 2]


def combine_costfunction_weighting(sourceweight, resampledtargetweight):
    """Mesh_registration::combine_costfunction_weighting, M/mesh_registration.cpp:849-869: the mean of the two weightings over
    the rows both have; the rows only the larger one has are kept"""
    a, b = np.atleast_2d(sourceweight), np.atleast_2d(resampledtargetweight)
    new = np.array(a if a.shape[0] >= b.shape[0] else b, dtype=np.float64)
    n = min(a.shape[0], b.shape[0])
    new[:n] = (a[:n] + b[:n]) / 2.0
    return new


def level_features(ops, timed, mesh, data, ico, sigma, varnorm, slot=None, excl=False, cutthr=(0.0, 0.0001)):
    """One data set of featurespace::initialise (M/featurespace.cpp:52-84) on a level's grid `ico`: metric_resample from its native mesh, smooth_data
    when sigma > 0, variance_normalise when varnorm.  Returns (features D x V(ico), mask).  excl (--excl): the mask is create_exclusion of the native
    data over the cut range cutthr (1 = kept, 0 = every feature inside the range: the medial wall of real data); resampling and smoothing leave it
    out and each hands back the mask on the grid, which replaces it (R/resampler.cpp:54-67, 168-230); the variance statistics run over vertices
    with mask > 0 and the others stay as they are (M/reg_tools.cpp:804-843).  Made afresh at every level from the native data, as the reference does.
    Without excl the ops are called exactly as before the option existed (an ops object need not know of masks) and the mask is None."""
    if not excl:
        f = timed("metric_resample", ops.metric_resample, *((mesh, data, ico) if slot is None else (mesh, data, ico, slot)))
        if sigma > 0.0:
            f = timed("smooth_data", ops.smooth_data, ico, f, sigma)
        return (ops.variance_normalise(f) if varnorm else f), None
    mask = ops.create_exclusion(data, cutthr[0], cutthr[1])
    f, mask = timed("metric_resample", lambda: ops.metric_resample(mesh, data, ico, excl=mask))
    if sigma > 0.0:
        f, mask = timed("smooth_data", lambda: ops.smooth_data(ico, f, sigma, excl=mask))
    if varnorm:
        f = ops.variance_normalise(f, excl=mask)
    return f, mask


class ReferenceCache:
    """The reference side of every level's feature preparation, prepared once for many registrations against one reference (cohort.py): per level
    the output of level_features for the reference data -- resampled, smoothed, variance normalised unless --IN / --INc postpone that, and the
    level-grid mask.  It depends on the reference, the level schedule, --excl / --cutthr and --INc, not on the subject: one cache serves runs that
    agree in those (the key of an entry holds them, so a run that differs computes its own).  Filled on first use and read afterwards; it owns its
    arrays -- copies on the host, never views of a context's reused result slot -- and is safe to share between threads, each with its own ops."""

    def __init__(self):
        self._lock = threading.Lock()
        self._entries = {}  # key -> [lock, (features, mask) or None]
        self.hits = 0
        self.fills = 0

    def get(self, key, compute):
        with self._lock:
            entry = self._entries.setdefault(key, [threading.Lock(), None])
        with entry[0]:  # a second thread that needs the entry being filled waits for it
            if entry[1] is None:
                f, m = compute()
                entry[1] = (np.array(f, dtype=np.float64, order="C"), None if m is None else np.array(m, dtype=np.float64, order="C"))
                for a in entry[1]:
                    if a is not None:
                        a.setflags(write=False)
                with self._lock:
                    self.fills += 1
            else:
                with self._lock:
                    self.hits += 1
            return entry[1]


def finish_features(ops, timed, feats, masks, intensity, varnorm):
    """The tail of featurespace::initialise (M/featurespace.cpp:75-83) over data sets that level_features has resampled and smoothed (varnorm=False):
    with intensity (--IN / --INc) every data set i >= 1 is histogram matched to data set 0, with the masks as they stand after smoothing (None
    without --excl / --INc); then variance_normalise of every data set when varnorm.  The reference's order is a quirk in a pairwise run, whose data
    sets are (input, reference): there the REFERENCE data is matched to the INPUT data.  Returns the list of feature matrices."""
    feats = list(feats)
    if intensity and len(feats) > 1:
        masked = masks[0] is not None
        feats[1:] = timed("histogram_match", ops.histogram_match, feats[1:], feats[0], list(masks[1:]) if masked else None, masks[0])
    if varnorm:
        feats = [ops.variance_normalise(f) if m is None else ops.variance_normalise(f, excl=m) for f, m in zip(feats, masks)]
    return feats


def composed_level_features(ops, timed, ico, meshes, datas, sigmas, exclude, intensity, varnorm, cutthr):
    """What ops.level_features_batch stands for, spelt out over the separate calls: level_features of every data set without variance normalisation
    (masks from the cut range when exclude), then finish_features -- matching of data sets 1.. to data set 0 when intensity, variance normalisation of
    each with its mask when varnorm.  Without intensity that is level_features with varnorm, data set by data set.  Returns (features, masks)."""
    prepared = [level_features(ops, timed, m, d, ico, s, False, None, exclude, cutthr) for m, d, s in zip(meshes, datas, sigmas)]
    masks = [p[1] for p in prepared]
    return finish_features(ops, timed, [p[0] for p in prepared], masks, intensity, varnorm), masks


def batched_pair_features(ops, timed, ico, li, lv, in_mesh, in_data, ref_mesh, ref_data, varnorm, excl, cutthr, intensity, cut, ref_cache):
    """A pairwise level's two feature matrices (input, reference) through ops.level_features_batch: one call over both data sets; with a ReferenceCache
    one call for the input data, the cache's entry (filled by one call for the reference data, under the key the unbatched loop uses) and
    finish_features over the two where --IN / --INc postpone the tail."""
    exclude, postponed = bool(excl or cut), bool(intensity or cut)
    sig_in, sig_ref = lv.get("sigma_in", 0.0), lv.get("sigma_ref", 0.0)
    if ref_cache is None:
        return timed("level_features", ops.level_features_batch, ico, [in_mesh, ref_mesh], [in_data, ref_data], [sig_in, sig_ref], exclude, intensity, varnorm, cutthr)[0]
    each = False if postponed else varnorm

    def one(mesh, data, sigma):
        f, m = timed("level_features", ops.level_features_batch, ico, [mesh], [data], [sigma], exclude, False, each, cutthr)
        return f[0], m[0]

    f_in, m_in = one(in_mesh, in_data, sig_in)
    key = (li, lv["data_order"], float(sig_ref), bool(each), exclude, tuple(float(c) for c in cutthr))
    f_ref, m_ref = ref_cache.get(key, lambda: one(ref_mesh, ref_data, sig_ref))
    feats = [f_in, f_ref]
    return finish_features(ops, timed, feats, [m_in, m_ref], intensity, varnorm) if postponed else feats


def transformed_data(ops, moved_mesh, in_data, ref_mesh, ref_data=None, *, excl=False, cutthr=(0.0, 0.0001), intensity=False):
    """save_transformed_data without its file I/O (M/mesh_registration.cpp:358-395): the native input data resampled from the registered input sphere
    (moved_mesh) onto the reference sphere.  excl (--excl): fresh masks from the native data keep the cut out of the resampling (:371-375).
    intensity (--IN / --INc): the native input data is first histogram matched to the native reference data (:376-380) -- this way round here, unlike
    in the levels' feature preparation -- with those masks under --excl only (--INc's cut alone makes none here).  Without intensity the ops are
    called exactly as before the option existed."""
    in_mask = ops.create_exclusion(in_data, cutthr[0], cutthr[1]) if excl else None
    if intensity:
        ref_mask = ops.create_exclusion(ref_data, cutthr[0], cutthr[1]) if excl else None
        in_data = ops.histogram_match([in_data], ref_data, [in_mask] if excl else None, ref_mask)[0]
    if excl:
        return ops.metric_resample(moved_mesh, in_data, ref_mesh, excl=in_mask)[0]
    return ops.metric_resample(moved_mesh, in_data, ref_mesh)


def project_start(ops, timed, ico_xyz, ico_tri, in_mesh, moved_in, cp_order):
    """project_CPgrid (M/mesh_registration.cpp:131-162) for a level that starts from a warp of the input sphere, in_mesh -> moved_in: the warp of
    the previous level carried to the input sphere (`incurrent`) or, at the first level, the --trans sphere.  The level's data grid is carried
    through it and unfolded; so is its control grid (warp_CPgrid, M/DiscreteModel.h:140-143) unless cp_order is None (a rigid level has no control
    grid).  Returns (data grid, control grid or None)."""
    moved = ops.mesh(timed("sphere_project_warp", ops.sphere_project_warp, ico_xyz, in_mesh, moved_in), ico_tri)
    cp_start = None
    if cp_order is not None:
        cp_xyz, cp_tri = ops.icosphere(cp_order)
        cpm = ops.mesh(timed("sphere_project_warp", ops.sphere_project_warp, cp_xyz, in_mesh, moved_in), cp_tri)  # warp_CPgrid
        timed("unfold", ops.unfold, cpm)
        cp_start = ops.coords(cpm)
    timed("unfold", ops.unfold, moved)
    return ops.coords(moved), cp_start


def usable_transformed(trans_xyz, in_xyz):
    """The --trans sphere as project_CPgrid looks at it at the first level (M/mesh_registration.cpp:136-145): None when it was not given or has the
    input sphere's coordinates (Mesh operator==, R/mesh.cpp:1285-1290: every coordinate within EPSILON = 1e-8), with the reference's warning.  It
    is taken as it is, not recentred and not rescaled (set_transformed); it must have the input sphere's vertex count, because sphere_project_warp
    reads it at the input sphere's vertex numbers (the reference would read out of bounds)."""
    if trans_xyz is None:
        return None
    trans_xyz = np.asarray(trans_xyz, dtype=np.float64)
    if trans_xyz.ndim != 2 or trans_xyz.shape[1] != 3 or len(trans_xyz) != len(in_xyz):
        raise ValueError("MeshREG ERROR:: the transformed mesh (--trans) has %d vertices, the input mesh has %d" % (len(trans_xyz), len(in_xyz)))
    if np.all(np.abs(trans_xyz - in_xyz) < 1e-8):
        print(" WARNING: transformed mesh has the same coordinates as the input mesh ", file=sys.stderr)
        return None
    return trans_xyz


def run_discrete_level(ops, target_xyz, target_tri, ref_feat, source_xyz, source_tri, src_feat, sph_reg, cp_order, *, sg_order=None,
                       iters=3, mciters=200, mcparam=0.8, seed=0, kind="univariate", simmeasure=2, rmode=3, labeldist=0.5,
                       rescale_labels=False, cost_params=None, timings=None, cp_start=None, in_weight=None, ref_weight=None,
                       optimiser="mcmc", icm_passes=5, converge=False, anat=None, speculate=True, mcmc_chains=1, fusion_trace=None):
    """Runs `iters` iterations of run_discrete_opt for one level.  optimiser: "mcmc" -- the reference's Monte Carlo optimiser over the
    unary and T x L^3 triplet tables (M/mcmc_opt.h:31-134) -- or "fusion": the label loop of Fusion::optimize (I/Fusion/Fusion.h:136-229: two
    sweeps over the labels, per label step 2 N unary and 8 T triplet costs -- ONE fusion-move call on the MI355X path --, nodes that the
    binary solve gives 1 take the label), which is how every HCP configuration drives the hot path (--dopt=HOCR).  The binary solve itself
    (ELC + FastPD, licence-restricted) is replaced by a stand-in (ops.fusion_step: iterated conditional modes, icm_passes passes): such a run
    exercises and times the path as HOCR would, its result is not the reference's optimum.  "fastpd": --regoption=1 as --dopt=FastPD drives it
    (M/mesh_registration.cpp:182-188): the unary table and the P x L x L pair tables (computePairwiseCosts), then a stand-in for FPD::FastPD
    (ops.pairwise_solve: iterated conditional modes over all labels).  "mplp_pairs" (an extension, taken only where ops.mplp_pairs is set): that pairwise model solved by MPLP over its unary
    and pair tables, `mciters` sweeps per iteration from the zero labelling and, with ops.mplp_round, ops.mplp_polish polish passes of
    the winner; on the device through the cost function where ops.mplp_gpu is set, over the fetched tables otherwise -- the same labelling.  "mplp" (an extension, not newMSM's): max-product linear programming over the
    MCMC optimiser's two tables, `mciters` sweeps per iteration from the zero labelling (api.mplp_optimise) -- deterministic, never
    worse than its start; the tables stay on the device where ops.mplp_gpu is set and the ops' cost function has mplp_optimise, otherwise they are
    fetched for the host literal (ops.mplp), which gives the same labelling; with ops.mplp_round the iteration rounds the final messages to a labelling
    after its sweeps (DESIGN.md 5.19 "Rounding"), on either route.  converge=True applies the reference's convergence test of a level
    (:204-213; the stand-in solves make its energies differ from the reference's, so it is off unless asked for).

    target / source: the reference and the moving sphere at the data resolution of this level (source_xyz = the sphere the
    moving features live on, sph_reg = its current registered position).  Returns (sph_reg, cp_xyz, energies, labelings).
    `timings` (optional dict) accumulates wall-clock seconds per phase.  cp_start: the control grid after warp_CPgrid (the
    warp of the previous level applied to it); the regular grid when None.  in_weight / ref_weight (rows x V, optional): the
    cost-function weightings of the moving and the reference data at this resolution (SPHin_CFWEIGHTING / SPHref_CFWEIGHTING);
    with both given every iteration resamples the reference weighting onto the moving sphere and averages the two
    (combine_weighting, M/mesh_registration.cpp:234-248), otherwise the weighting is all ones.
    mcmc_chains (optimiser "mcmc"): every iteration runs this many chains from the one labelling, chain k seeded with seed + it + 1000003 k
    (api.chain_seeds), and keeps the labelling with the lowest table energy (ops' cost.mcmc_optimise_chains with ops.mcmc_gpu, ops.mcmc_chains
    over the fetched tables without: the same labelling); 1 is the single run.
    speculate (fusion loop): queue the next label step's evaluations while the host solves the current one (ops' cost.prefetch_octets, if it has one).
    Where ops.fusion_mplp is set (an extension) the binary problem of a label step is solved by MPLP instead of ops.fusion_step: with
    ops.mplp_gpu on the device behind the step's own kernel (the ops' cost.fusion_mplp_step; nothing is left for the host to solve meanwhile, so no
    step is queued ahead), otherwise by the host literal over the fetched octets (ops.fusion_mplp_step), speculation as before -- the same
    labellings on either route, with or without speculate.  fusion_trace (optional list) receives (iteration, label, api.FusionMplp) per solved step.
    anat (rmode 4 / 5, aMSM): dict(order, in_anat, in_mesh, ref_anat, ref_mesh) -- --anatgrid of this level and the input / reference anatomical
    surfaces (V x 3) with the spheres (ops meshes) whose vertices they share (MESHES[0] / MESHES[1]).  initialize_level (M/mesh_registration.cpp:
    91-99) then prepares the anatomical regulariser: resample_anatomy (:250-332: the control grid retessellated to anatomical resolution with the
    face neighbourhoods -> NEARESTFACES, _ANATbaryweights, the input anatomy resampled onto it), the reference anatomy resampled the same way,
    set_anatomical_meshspace / set_anatomical_neighbourhood.  (setupCostFunction's reset_anatomical, M/DiscreteCostFunction.cpp:85-100, computes
    _aSOURCEtrans and MAXstrain, which nothing reads: not evaluated.)"""
    if sg_order is None:
        sg_order = cp_order + 2
    cost_params = dict(cost_params or {})
    clock = timings if timings is not None else {}

    def timed(name, fn, *a):
        t0 = time.perf_counter()
        out = fn(*a)
        clock[name] = clock.get(name, 0.0) + time.perf_counter() - t0
        return out

    # --- initialize_level / Initialize(CONTROL)
    cp_xyz, cp_tri = ops.icosphere(cp_order)
    target = ops.mesh(target_xyz, target_tri, ref_feat)
    source = ops.mesh(source_xyz, source_tri)
    cpgrid = ops.mesh(cp_xyz, cp_tri)
    maxsep, mvdmax = ops.cp_spacings(cpgrid, cp_xyz, cp_tri)
    samples, barycentres = ops.label_sampling_grid(sg_order, labeldist * mvdmax)
    centre = samples[0]
    pairwise = optimiser in ("fastpd", "mplp_pairs")  # --regoption=1: the model lists pairs instead of triplets (M/DiscreteModel.cpp:40,98-101,258-259)
    if pairwise and rmode != 1:
        raise ValueError("MeshREG ERROR:: you cannot run higher order clique regularisers with fastPD ")  # M/mesh_registration.cpp:759-760
    if optimiser == "mplp_pairs" and not getattr(ops, "mplp_pairs", False):  # an extension, opt-in like the others: the ops must have asked for it
        raise ValueError("optimiser \"mplp_pairs\" (MPLP over the pair tables, an extension) needs ops.mplp_pairs: ProductOps(mplp_pairs=True)")
    triplets = None if pairwise else ops.estimate_triplets(cpgrid, cp_tri)
    pairs = ops.estimate_pairs(cpgrid, cp_tri, len(cp_xyz)) if pairwise else None
    cost = ops.cost(kind, simmeasure, rmode, cost_params, target, source, cpgrid, src_feat)  # set_meshes: _ORIG, _oCPgrid
    cost.set_spacings(maxsep, mvdmax)
    if rmode in (4, 5):
        if anat is None:  # M/mesh_registration.cpp:100-104
            raise ValueError("--regoption 4 has been removed from newMSM. Use --regoption 3 for spherical mesh regularisation or --regoption 5 for anatomical mesh "
                             "regularisation." if rmode == 4 else
                             "--regoption 5 requires anatomical meshes. Use --regoption 3 for spherical mesh regularisation or provide anatomical meshes.")
        if pairwise:
            raise ValueError("MeshREG ERROR:: you cannot run higher order clique regularisers with fastPD ")
        grid = ops.resample_anatomy_grid(cp_xyz, cp_tri, max(0, anat["order"] - cp_order))     # ANAT_ico, _ANATbaryweights, NEARESTFACES
        anat_orig = timed("surface_resample", ops.surface_resample, anat["in_anat"], anat["in_mesh"], grid["sphere_xyz"])    # ANAT_orig (:323)
        anat_target = timed("surface_resample", ops.surface_resample, anat["ref_anat"], anat["ref_mesh"], grid["sphere_xyz"])  # ANAT_target (:93)
        cost.set_triplets(triplets)  # NEARESTFACES is indexed by triplet = control triangle
        cost.set_anatomical(ops.mesh(grid["sphere_xyz"], grid["sphere_tri"]), anat_target, anat_orig, grid)
    m_iter, m_scale = 1, 1.0
    energies, labelings = [], []
    energy = 0.0
    sph_reg = np.array(sph_reg, dtype=np.float64)
    if cp_start is not None:
        cp_xyz = np.array(cp_start, dtype=np.float64)
    for it in range(iters):
        # --- reset_meshspace + setupCostFunction
        ops.set_coords(source, sph_reg)
        if in_weight is not None and ref_weight is not None:  # setupCostFunctionWeighting(combine_weighting())
            resampled = timed("metric_resample", ops.metric_resample, target, ref_weight, source)
            cost.set_cfweight(combine_costfunction_weighting(in_weight, resampled))
        cost.reset_source(source)
        ops.set_coords(cpgrid, cp_xyz)
        cost.reset_cpgrid(cpgrid)
        rot = ops.cp_rotations(centre, cp_xyz)
        if rescale_labels:
            labels, m_scale = ops.rescale_sampling_grid(samples, m_scale)
        elif m_iter % 2 == 0:
            labels = samples
        else:
            labels = barycentres
        cost.set_labels(labels, rot)
        timed("get_source_data", cost.get_source_data)
        if pairwise:
            cost.set_pairs(pairs)
        else:
            cost.set_triplets(triplets)
        m_iter += 1
        mcmc_gpu = optimiser == "mcmc" and getattr(ops, "mcmc_gpu", False)  # both tables stay on the device (msm_cost_mcmc_optimise)
        mplp_gpu = optimiser == "mplp" and getattr(ops, "mplp_gpu", False) and hasattr(cost, "mplp_optimise")  # the same for msm_cost_mplp_optimise
        mplp_pairs_gpu = optimiser == "mplp_pairs" and getattr(ops, "mplp_gpu", False) and hasattr(cost, "mplp_pairs_optimise")  # msm_cost_mplp_pairs_optimise
        unary = None if mcmc_gpu or mplp_gpu or mplp_pairs_gpu else timed("unary_table", cost.unary_table)
        labeling = np.zeros(len(cp_xyz), dtype=np.int32)  # resetLabeling
        if optimiser == "fusion":  # --- Fusion::optimize: computeUnaryCosts, then per label step the 8 T combinations
            nodes = np.arange(len(cp_xyz))
            L = len(labels)
            steps = [(sweep, label) for sweep in range(2) for label in range(L)]
            prefetch = getattr(cost, "prefetch_octets", None) if speculate else None
            fusion_mplp = bool(getattr(ops, "fusion_mplp", False))
            fusion_gpu = fusion_mplp and getattr(ops, "mplp_gpu", False) and hasattr(cost, "fusion_mplp_step")  # msm_cost_fusion_mplp_step
            for k, (sweep, label) in enumerate(steps):
                if not np.any(labeling != label):
                    continue
                if fusion_gpu:  # --- octets, unary gather and the MPLP solve in one go on the device
                    r = timed("optimiser", cost.fusion_mplp_step, labeling, label, ops.fusion_sweeps, ops.fusion_polish)
                    if fusion_trace is not None:
                        fusion_trace.append((it, label, r))
                    labeling = np.where((r.x == 1) & (labeling != label), label, labeling).astype(np.int32)
                    continue
                octets = timed("fusion_moves", cost.triplet_octets, labeling, label)
                if prefetch is not None:
                    # While the host solves this step the GPU would idle; most steps of a converging level change no label, and then the next step's
                    # evaluations are a function of what is known now: queue them (a hint: the results do not depend on it, a step whose labeling did
                    # change is evaluated afresh)
                    nxt = next((lb for _, lb in steps[k + 1:] if np.any(labeling != lb)), None)
                    if nxt is not None:
                        timed("fusion_prefetch", prefetch, labeling, nxt)
                unary2 = np.stack([unary[labeling, nodes], unary[label]], axis=1)
                if fusion_mplp:  # --- the same solve by the host literal
                    r = timed("optimiser", ops.fusion_mplp_step, unary2, octets, triplets)
                    if fusion_trace is not None:
                        fusion_trace.append((it, label, r))
                    x = r.x
                else:
                    x = timed("optimiser", ops.fusion_step, unary2, octets, triplets, icm_passes)
                labeling = np.where((x == 1) & (labeling != label), label, labeling).astype(np.int32)
        elif mplp_pairs_gpu:  # --- MPLP over the pair tables, tables and sweeps on the device: the labeling of the branch below, bit for bit
            labeling = timed("optimiser", cost.mplp_pairs_optimise, labeling, mciters, ops.mplp_polish if getattr(ops, "mplp_round", False) else 0)
        elif optimiser == "mplp_pairs":  # --- the same over fetched tables: computeUnaryCosts, computePairwiseCosts, the host literal and its polish
            paircosts = timed("pairwise_table", cost.pairwise_table)
            labeling = timed("optimiser", getattr(ops, "mplp_pairs_solve", _mplp_pairs_host), unary, paircosts, pairs, labeling, mciters)
        elif pairwise:  # --- FastPD: computeUnaryCosts, computePairwiseCosts, FPD::FastPD(model, 100) (M/mesh_registration.cpp:182-188)
            paircosts = timed("pairwise_table", cost.pairwise_table)
            labeling = timed("optimiser", ops.pairwise_solve, unary, paircosts, pairs, 100)
        elif mplp_gpu:  # --- MPLP with the tables and the sweeps on the device: the labeling of the branch below, bit for bit
            if getattr(ops, "mplp_round", False):  # the sweeps, then the rounding of their messages (msm_cost_mplp_round)
                labeling = timed("optimiser", cost.mplp_round, labeling, mciters, ops.mplp_polish)
            else:
                labeling = timed("optimiser", cost.mplp_optimise, labeling, mciters)
        elif optimiser == "mplp":  # --- MPLP: computeUnaryCosts, computeTripletCosts, the host literal
            tcosts = timed("triplet_table", cost.triplet_table)
            labeling = timed("optimiser", getattr(ops, "mplp", _mplp_host), unary, tcosts, triplets, labeling, mciters)
        elif mcmc_gpu:  # --- MCMC with the tables and the sweeps on the device: the labeling of the branch below, bit for bit
            if mcmc_chains > 1:
                labeling = timed("optimiser", cost.mcmc_optimise_chains, labeling, mcparam, mciters, api.chain_seeds(seed, it, mcmc_chains))
            else:
                labeling = timed("optimiser", cost.mcmc_optimise, labeling, mcparam, mciters, seed + it)
        else:  # --- MCMC: computeUnaryCosts, computeTripletCosts, optimise
            tcosts = timed("triplet_table", cost.triplet_table)
            if mcmc_chains > 1:
                labeling = timed("optimiser", ops.mcmc_chains, unary, tcosts, triplets, labeling, mcparam, mciters, api.chain_seeds(seed, it, mcmc_chains))
            else:
                labeling = timed("optimiser", ops.mcmc, unary, tcosts, triplets, labeling, mcparam, mciters, seed + it)
        newenergy = timed("total_cost", cost.total, labeling)
        # the level's convergence test (M/mesh_registration.cpp:204-213): from the fourth iteration on, every second one, not for MCMC; the
        # iteration that triggers it is not applied
        if converge and it > 2 and (it - 1) % 2 == 0 and energy - newenergy < 0.001 and optimiser != "mcmc":
            break
        energy = newenergy
        energies.append(newenergy)
        labelings.append(labeling)
        # --- applyLabeling, warp the source through the control grid move, unfold both
        new_cp = apply_labeling(rot, labels, labeling)
        # (the source mesh holds sph_reg since the top of the iteration: it is warped where it lies; cpgrid still holds the previous grid)
        timed("sphere_project_warp", ops.warp_mesh, source, cpgrid, new_cp)
        ops.set_coords(cpgrid, new_cp)
        timed("unfold", ops.unfold, cpgrid)
        cp_xyz = ops.coords(cpgrid)
        timed("unfold", ops.unfold, source)
        sph_reg = ops.coords(source)
    return sph_reg, cp_xyz, energies, labelings


def run_multiresolution(ops, in_xyz, in_tri, in_data, ref_xyz, ref_tri, ref_data, levels, *, varnorm=False, timings=None, in_cfweight=None,
                        ref_cfweight=None, labelings_out=None, in_anat=None, ref_anat=None, trans_xyz=None, excl=False, cutthr=(0.0, 0.0001),
                        intensity=False, cut=False, ref_cache=None, **level_kw):
    """Mesh_registration::run_multiresolutions (M/mesh_registration.cpp:30-50) for DISCRETE and RIGID levels without file I/O:

    per level  featurespace::initialise (M/featurespace.cpp:39-86: metric_resample of both data sets onto the level's
               icosphere, smooth_data, variance_normalise), project_CPgrid (M/mesh_registration.cpp:131-162: the warp of the
               previous level carried to the new data grid and control grid, unfold) and run_discrete_opt;
    at the end transform (:352-356): the input sphere moved through the final warp ("sphere.reg").

    in_* / ref_*: the input and reference spheres (radius 100) with their D x V data.  levels: dicts with data_order, cp_order
    and optionally sg_order, sigma_in, sigma_ref, iters, mciters, cost_params; a level with method="RIGID" (config.levels_from_config(...,
    rigid=True)) runs Rigid_cost_function instead (ops.rigid_level): its regs entry is the rotated data grid, its energies entry the optimiser's
    trace, and it adds no labelings.  in_cfweight / ref_cfweight (rows x V on the
    input / reference sphere, optional): cost-function weightings, brought to each level's grid by nearest-neighbour
    interpolation (downsample_cfweighting, M/mesh_registration.cpp:334-350).  labelings_out (optional list): receives every iteration's labeling, level
    after level (the parity tests compare the optimiser's decisions of two runs).  in_anat / ref_anat (V x 3 on the vertices of the input /
    reference sphere; both or none, CLI/newmsm.cpp:40-45): the anatomical surfaces of a --regoption=5 (aMSM) run; a level's "anat_order" is its
    --anatgrid.  recentre() of the regular spheres
    (a shift of ~1e-15) is not applied.
    trans_xyz (V(input) x 3, optional; --trans): the input sphere as an earlier registration left it (its sphere.reg), taken as it is.  Only the
    first level looks at it (project_CPgrid, M/mesh_registration.cpp:136-145): its data grid and control grid start carried through input sphere ->
    trans_xyz, which is what every later level does with the warp of the level before it, so the run continues the earlier one and sphere_reg is
    the composition.  A first level that is RIGID has no control grid to carry (the reference would call warp_CPgrid on a model that does not exist
    yet); its data grid is projected.  Coordinates equal to the input sphere's: the reference's warning, and the run goes on without it.
    excl, cutthr (--excl, --cutthr): exclusion masks from the cut thresholds in every level's feature preparation (level_features).  They do not
    enter the cost function: combine_weighting (M/mesh_registration.cpp:234-248) returns ones unless both weightings are given, and with both,
    downsample_cfweighting (:334-350) would read the level-grid mask at vertex numbers of the weightings' own meshes -- refused.
    intensity, cut (--IN / --INc; config.levels_from_config(..., histmatch=True)): in every level's feature preparation, RIGID levels included, the
    reference data is histogram matched to the input data after both are resampled and smoothed and before variance normalisation (finish_features:
    the reference's order, a quirk); cut (--INc) makes the exclusion masks exist as --excl does (M/featurespace.cpp:61).  The final resampling is
    the caller's (transformed_data).
    ref_cache (optional, a ReferenceCache): the reference data's level_features output is taken from it, and put there by the first run that needs
    it, instead of being computed at every level of every run; everything after it (finish_features, the level's target mesh) stays this run's own.
    Without it every call is what it was before the argument existed.
    Returns (sphere_reg, per-level registered data grids, per-level energies)."""
    if excl and in_cfweight is not None and ref_cfweight is not None:
        raise ValueError(EXCL_WITH_WEIGHTINGS)
    clock = timings if timings is not None else {}

    def timed(name, fn, *a):
        t0 = time.perf_counter()
        out = fn(*a)
        clock[name] = clock.get(name, 0.0) + time.perf_counter() - t0
        return out

    in_xyz = np.asarray(in_xyz, dtype=np.float64)
    trans_xyz = usable_transformed(trans_xyz, in_xyz)
    in_mesh, ref_mesh = ops.mesh(in_xyz, in_tri), ops.mesh(ref_xyz, ref_tri)
    sph_reg_prev, prev_order, regs, all_energies = None, None, [], []
    # the two data matrices go up once per level: in page-locked memory for the run, their uploads skip the staging blocks (ProductOps.pin; absent elsewhere)
    pins = []
    try:
        if hasattr(ops, "pin"):
            for which in (0, 1):
                token, arr = ops.pin(in_data if which == 0 else ref_data)
                pins.append(token)
                if which == 0:
                    in_data = arr
                else:
                    ref_data = arr
        return _run_levels(ops, clock, timed, in_xyz, in_mesh, ref_mesh, in_data, ref_data, levels, varnorm, in_cfweight, ref_cfweight, labelings_out, in_anat,
                           ref_anat, ref_xyz, level_kw, sph_reg_prev, prev_order, regs, all_energies, trans_xyz, excl, cutthr, intensity, cut, ref_cache)
    finally:
        for t in pins:
            ops.unpin(t)


def _run_levels(ops, clock, timed, in_xyz, in_mesh, ref_mesh, in_data, ref_data, levels, varnorm, in_cfweight, ref_cfweight, labelings_out, in_anat, ref_anat,
                ref_xyz, level_kw, sph_reg_prev, prev_order, regs, all_energies, trans_xyz=None, excl=False, cutthr=(0.0, 0.0001), intensity=False, cut=False, ref_cache=None):
    """the level loop of run_multiresolution (see there)"""
    for li, lv in enumerate(levels):
        rigid = lv.get("method") == "RIGID"
        ico_xyz, ico_tri = ops.icosphere(lv["data_order"])
        ico = ops.mesh(ico_xyz, ico_tri)
        feats, masks = [], []
        batched = getattr(ops, "features_gpu", False)  # featurespace::initialise in one call: the bytes of the loop below
        data_sets = ((in_mesh, in_data, lv.get("sigma_in", 0.0), "in"), (ref_mesh, ref_data, lv.get("sigma_ref", 0.0), "ref"))
        if batched:
            feats = batched_pair_features(ops, timed, ico, li, lv, in_mesh, in_data, ref_mesh, ref_data, varnorm, excl, cutthr, intensity, cut, ref_cache)
            data_sets = ()
        for mesh, data, sigma, slot in data_sets:
            # (a level's matrices are consumed -- uploaded by the cost function and the target mesh -- before the next level asks for its own: the
            # result slots are reused from level to level)
            if intensity or cut:  # resample and smooth only: matching and variance normalisation follow when both data sets are there
                args = (False, slot, excl or cut, cutthr)
            else:
                args = (varnorm, slot, excl, cutthr)
            if slot == "ref" and ref_cache is not None:
                key = (li, lv["data_order"], float(sigma), bool(args[0]), bool(args[2]), tuple(float(c) for c in cutthr))
                f, m = ref_cache.get(key, lambda: level_features(ops, timed, mesh, data, ico, sigma, *args))
            else:
                f, m = level_features(ops, timed, mesh, data, ico, sigma, *args)
            if intensity or cut:
                masks.append(m)
            feats.append(f)
        if (intensity or cut) and not batched:
            feats = finish_features(ops, timed, feats, masks, intensity, varnorm)
        # project_CPgrid: the warp this level starts from, as the input sphere moved through it -- the previous level's, or --trans at the first
        if sph_reg_prev is None:
            moved_in = trans_xyz
        else:
            prev_xyz, prev_tri = ops.icosphere(prev_order)
            moved_in = timed("sphere_project_warp", ops.sphere_project_warp, in_xyz, ops.mesh(prev_xyz, prev_tri), sph_reg_prev)  # incurrent
        if moved_in is None:  # level 1, no transformed mesh: project_CPgrid only unfolds the (regular) data grid
            moved = ops.mesh(ico_xyz, ico_tri)
            timed("unfold", ops.unfold, moved)
            sph_in, cp_start = ops.coords(moved), None
        else:  # (a rigid level has no control grid: no warp_CPgrid)
            sph_in, cp_start = project_start(ops, timed, ico_xyz, ico_tri, in_mesh, moved_in, None if rigid else lv["cp_order"])
        if rigid:  # Rigid_cost_function on the level's featurespace: the grid rotated as a whole, no labelings
            sph_reg, trace = timed("rigid", ops.rigid_level, ico_xyz, ico_tri, feats[1], ico_xyz, ico_tri, feats[0], sph_in, lv["iters"], lv["simmeasure"],
                                   lv["stepsize"], lv["gradsampling"])
            regs.append(sph_reg)
            all_energies.append(trace)
            sph_reg_prev, prev_order = sph_reg, lv["data_order"]
            continue
        kw = dict(level_kw)
        kw.update({k: lv[k] for k in ("sg_order", "iters", "mciters", "mcparam", "cost_params", "kind", "rescale_labels", "optimiser", "simmeasure", "rmode",
                                      "converge") if k in lv})
        if in_anat is not None or ref_anat is not None:
            if in_anat is None or ref_anat is None:
                raise ValueError("Error: must supply both anatomical meshes or none")  # CLI/newmsm.cpp:41-43
            if len(in_anat) != len(in_xyz) or len(ref_anat) != len(np.asarray(ref_xyz)):
                raise ValueError("MeshREG ERROR:: input/reference anatomical mesh resolution is inconsistent with input/reference spherical mesh resolution.")
            kw["anat"] = dict(order=lv.get("anat_order", lv["cp_order"] + 2), in_anat=np.asarray(in_anat, dtype=np.float64), in_mesh=in_mesh,
                              ref_anat=np.asarray(ref_anat, dtype=np.float64), ref_mesh=ref_mesh)
        if in_cfweight is not None and ref_cfweight is not None:
            kw["in_weight"] = ops.nearest_neighbour(in_mesh, in_cfweight, ico_xyz)
            kw["ref_weight"] = ops.nearest_neighbour(ref_mesh, ref_cfweight, ico_xyz)
        sph_reg, _, energies, labelings = run_discrete_level(ops, ico_xyz, ico_tri, feats[1], ico_xyz, ico_tri, feats[0], sph_in, lv["cp_order"],
                                                             cp_start=cp_start, timings=clock, **kw)
        if labelings_out is not None:
            labelings_out.extend(labelings)
        regs.append(sph_reg)
        all_energies.append(energies)
        sph_reg_prev, prev_order = sph_reg, lv["data_order"]
    last_xyz, last_tri = ops.icosphere(levels[-1]["data_order"])
    sphere_reg = timed("sphere_project_warp", ops.sphere_project_warp, in_xyz, ops.mesh(last_xyz, last_tri), sph_reg_prev)
    return sphere_reg, regs, all_energies
