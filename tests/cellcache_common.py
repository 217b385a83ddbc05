"""Shared by tests/test_cellcache_rules.py (the host emulation's rows) and tests/test_gpu_cellcache.py (the engine's rows): a cell's whole row --
the reference's spans (debug_cellcache) and every array the row keeps beside them (debug_cellcache_array) -- against the oracle
(oracle_py.cellcache + cellcache_extra), the arrays that are re-orderings of others against those others, and the cell states whose first
cells are edges.

A "view" is anything with debug_cellcache(c) and debug_cellcache_array(c, name): an engine.Engine, or hostemu_binding.CellCacheView."""
import numpy as np

from artis_amd import abi, synth

# The builds whose options change a body of the population (the `#if`s and constant conditions of physics.h between "cell-cache population" and
# the cooling guides, with the expansion opacities):
#   classic                 USE_LUT_PHOTOION, LTEPOP_EXCITATION_USE_TJ, PHIXS_CLASSIC_NO_INTERPOLATION, MINPOP 1e-30: the base
#   kilonova_lte            PHIXS_CLASSIC_NO_INTERPOLATION off, MINPOP 1e-40, the 200-point table grid
#   nltenebular             no USE_LUT_PHOTOION (coefficients and level populations of the host), MULTIBIN_RADFIELD_MODEL_ON and
#                           DETAILED_BF_ESTIMATORS_ON (radiative excitation from the binned field), NT_ON (k_nt_cells, non-thermal rates in the records)
#   nltenebular_lineest     DETAILED_LINE_ESTIMATORS_ON (Jb_lu_normed in the radiative excitation rates)
#   christinenonthermal     NT_EXCITATION_ON off (nt_excitation_ratecoeff is constant 0), 64 radiation-field bins
#   nltewithoutnonthermal   BFCOOLING_USELEVELPOPNOTIONPOP (the bound-free cooling terms weigh with the upper level's population); not in the
#                           list the work started from: no other build flips that switch
#   kilonova_expopac        the expansion opacities without RPKT_BB_THERMALISATION (k_expopac)
#   classic_expopac_therm   ... and with it (k_expopac_planck)
# Two more flip none of those switches against a build above and are kept because they cost a second each and compile another table grid into
# the interpolations of the bound-free coefficients: nltephotospheric (nltenebular with TABLESIZE 100 from 3500 K) and ci_kilonova_xcom
# (kilonova_lte with TABLESIZE 20 up to 20000 K). ci_kilonova_xcom's mean atomic weights (USE_CALCULATED_MEANATOMICWEIGHT) reach no body of the
# population: elem_numberdens() is read there by populate_nt_cell() alone, and no build has both NT_ON and the mean weights.
BUILDS = ("classic", "kilonova_lte", "nltenebular", "nltenebular_lineest", "nltephotospheric", "christinenonthermal", "nltewithoutnonthermal",
          "ci_kilonova_xcom", "kilonova_expopac", "classic_expopac_therm")
EDGE_BUILDS = ("classic", "nltenebular", "kilonova_expopac")

MAIN_F64 = ("levelpops", "maprocessrates", "matrans", "allcont_nnlevel", "allcont_departure", "allcont_edgepart", "corrphotoioncoeff",
            "cooling_contrib", "ion_cooling_contribs", "chi_ff_nnionpart")
EXTRA_F64 = ("line_dpop", "bf_radrecomb", "bf_colrecomb", "bf_colion", "bf_cooling", "ion_cooling_C", "expansionopacity_planck_cumulative",
             "nt_ionratecoeff", "nt_ionenrate_cum")
F64_BAR = 1e-12          # the bar of test_cellcache_matches_oracle: |a - b| / max(|a|, |b|, 1e-300)
F32_ULP = 2.0 ** -23     # expansionopacities are stored as float32: one unit in the last place
CELL_THICK = 1           # ARTIS_CELL_THICK
THICK_BELOW_V = 1.1e9    # cm/s: on 4^3 cells the eight innermost (centres at 1.04e9) are thick


def expected_arrays(options: str) -> set:
    """the arrays of abi.CC_ARRAYS a row has in this build, with the atomic data and the default configuration the tests use (line_dpop kept,
    guides on, expansion tables made by the engine)"""
    have = set(abi.CC_ARRAYS) - {"expansionopacities", "expansionopacity_planck_cumulative", "nt_ionratecoeff", "nt_ionenrate_cum"}
    if "expopac" in options:
        have.add("expansionopacities")
        if options.endswith("_therm"):
            have.add("expansionopacity_planck_cumulative")
    if options in abi.NEBULAR_FAMILY:
        have |= {"nt_ionratecoeff", "nt_ionenrate_cum"}
    return have


def view_row(view, c: int, options: str) -> dict:
    """cell c's row from both entry points; an array the build should not have must be refused"""
    row = dict(view.debug_cellcache(c))
    have = expected_arrays(options)
    for name in abi.CC_ARRAYS:
        if name in have:
            got = view.debug_cellcache_array(c, name)
            if name == "allcont_keepbits":
                row["allcont_keepbits_row"] = got  # (the padded row; debug_cellcache's "allcont_keepbits" are its first ceil(n / 64) words)
            else:
                row[name] = got
        else:
            try:
                view.debug_cellcache_array(c, name)
            except Exception:
                continue
            raise AssertionError(f"{options}: {name} should not exist in this build")
    return row


def oracle_row(oracle, model, cs, ts, c: int, options: str) -> dict:
    ref = dict(oracle.cellcache(model, cs, ts, c, preset=options))
    ref.update(oracle.cellcache_extra(model, cs, ts, c, preset=options))
    return ref


def reldiff(x, y, scale=None) -> float:
    """max |x - y| / max(|x|, |y|, 1e-300); scale: measured against it instead where it is larger (a difference of two terms: the larger term)"""
    x, y = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64))
    assert x.shape == y.shape, (x.shape, y.shape)
    if x.size == 0:
        return 0.0
    assert np.isfinite(x).all() and np.isfinite(y).all(), "non-finite entries"
    denom = np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-300)
    if scale is not None:
        denom = np.maximum(denom, np.asarray(scale, dtype=np.float64))
    return float((np.abs(x - y) / denom).max())


def check_against_oracle(row: dict, ref: dict, model, cs, c: int, options: str, exact: bool, what: str, worst: dict = None):
    """Every entry of every array of `row` that the oracle restates. exact: equal bits (the host emulation); else the bars above (the GPU).
    worst: name -> the largest relative difference seen so far (updated before asserting, so a run can report what it measured).

    One array is a difference of nearly equal terms and is measured against the larger term, which the oracle returns beside it: line_dpop =
    B_lu n_l - B_ul n_u, where the two level populations the GPU forms (each within rounding of the oracle's) can cancel to any fraction of
    themselves -- in thermodynamic equilibrium at a line's own temperature to nothing. No other array needs it: the departure ratios and
    stimulated-correction factors of the continua are products and quotients, the rates and cooling terms sums of non-negative terms."""
    d = model.d
    nbf, nw = int(d["nbfcontinua"]), (int(d["nbfcontinua"]) + 63) // 64
    assert np.array_equal(row["allcont_keepbits"][:nw], ref["allcont_keepbits"][:nw]), f"{what}: allcont_keepbits"

    def one(name, got, want, scale=None, bar=F64_BAR):
        assert np.shape(got) == np.shape(want), f"{what}: {name} {np.shape(got)} {np.shape(want)}"
        if exact:
            assert np.array_equal(got, want), f"{what}: {name}"
            return
        r = reldiff(got, want, scale)
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), r)
        assert r <= bar, f"{what}: {name} {r:.3e}"

    for name in MAIN_F64:
        n = {"allcont_nnlevel": nbf, "allcont_departure": nbf, "allcont_edgepart": nbf}.get(name)
        got, want = np.atleast_1d(row[name]), np.atleast_1d(ref[name])
        one(name, got[:n] if n is not None else got, want[:n] if n is not None else want)
    for name in EXTRA_F64:
        assert (name in row) == (name in expected_arrays(options)), f"{what}: {name}"
        if name not in row:
            continue
        if name == "expansionopacity_planck_cumulative" and name not in ref:
            continue  # (a thick cell: below)
        one(name, row[name], ref[name], scale=np.abs(ref["line_dpop_terms"]).max(axis=1) if name == "line_dpop" else None)
    if "expansionopacities" in row:
        if int(cs.d["thick"][c]) == CELL_THICK:  # update_grid.cc:655: no tables for a thick cell; the engine's rows stay as allocated, zero
            assert "expansionopacities" not in ref, what
            assert not row["expansionopacities"].any(), f"{what}: expansionopacities of a thick cell"
            if "expansionopacity_planck_cumulative" in row:
                assert not row["expansionopacity_planck_cumulative"].any(), f"{what}: expansionopacity_planck_cumulative of a thick cell"
        else:
            assert row["expansionopacities"].dtype == np.float32 and ref["expansionopacities"].dtype == np.float32
            one("expansionopacities", row["expansionopacities"], ref["expansionopacities"], bar=F32_ULP)
    else:
        assert "expansionopacities" not in ref, f"{what}: the oracle has expansion tables, the row none"


def check_derived(row: dict, model, guide_row, what: str):
    """The arrays of a row that re-order or pack others of the SAME row, exactly: the padded bitmap, allcont_pair, the list of kept continua, the
    counts below each bitmap word, the pairs in list order; and the cooling guides against physics.h cool_guide_entry() on the row's own two
    cumulative lists (guide_row: hostemu_binding.cool_guide_row)."""
    d = model.d
    nbf, nw = int(d["nbfcontinua"]), (int(d["nbfcontinua"]) + 63) // 64
    bits = row["allcont_keepbits_row"]
    assert len(bits) % 4 == 0 and len(bits) >= nw, f"{what}: nkeepwords {len(bits)}"
    assert np.array_equal(bits[:nw], row["allcont_keepbits"][:nw]), f"{what}: the two views of allcont_keepbits"
    set_bits = np.flatnonzero(np.unpackbits(bits.view(np.uint8), bitorder="little"))
    assert set_bits.size == 0 or set_bits.max() < nbf, f"{what}: a keep bit at or above nbfcontinua"
    pair = row["allcont_pair"]
    assert pair.shape == (nbf, 2)
    assert np.array_equal(pair[:, 0], row["allcont_nnlevel"][:nbf]) and np.array_equal(pair[:, 1], row["allcont_edgepart"][:nbf]), f"{what}: allcont_pair"
    nkept = set_bits.size
    # (the list and the pairs in its order have a place for every continuum; the population writes the first nkept)
    assert np.array_equal(row["allcont_keptlist"][:nkept], set_bits.astype(np.int32)), f"{what}: allcont_keptlist"
    assert np.array_equal(row["allcont_keptpair"][:nkept], pair[set_bits]), f"{what}: allcont_keptpair"
    popcount = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(len(bits), 64).sum(axis=1)
    assert np.array_equal(row["allcont_keepprefix"], (np.cumsum(popcount) - popcount).astype(np.int32)), f"{what}: allcont_keepprefix"
    want = guide_row(model, np.atleast_1d(row["ion_cooling_contribs"]), row["cooling_contrib"])
    assert row["cool_guide"].dtype == np.uint16 and want.dtype == np.uint16 and len(want) > 0
    assert np.array_equal(row["cool_guide"], want), f"{what}: cool_guide"


# Atomic data that take the loop trips `small` never takes (synth.PRESETS entries: elements, levels per ion, line fraction, cross-section points)
SHAPES = {
    # more than 4096 continua, not a multiple of 64: k_keptlist's second trip over the bitmap words, a last word that is partly empty
    "manycont": ([(26, 1, 5), (27, 1, 5), (28, 1, 5)], 350, 0.1, 12),
    # 3 continua: less than one wave
    "one_ion": ([(14, 1, 2)], 3, 1.0, 12),
    # directions of more than 256 transitions: k_matrans sums them 64 terms at a time, k_mafilter_long writes their filters
    "longdir": ([(26, 1, 2)], 420, 0.7, 12),
    # more than 16 items for the rows of 16 lanes of k_macroatom_recomb and the cooling chain, more than 16 ions
    "wide": ([(8, 1, 4), (14, 1, 5), (26, 1, 5), (28, 1, 5)], 40, 0.3, 12),
}


def assert_shape(name: str, model):
    """the property a shape is there for, from the model's own fields (a change of synth cannot silently un-test it)"""
    d = model.d
    nbf = int(d["nbfcontinua"])
    if name == "manycont":
        assert nbf > 4096 and nbf % 64 != 0 and (nbf + 63) // 64 > 64
    elif name == "one_ion":
        assert nbf == 3
    elif name == "longdir":
        assert max(d["level_ndowntrans"]) > 256 and max(d["level_nuptrans"]) > 256
    elif name == "wide":
        # k_macroatom_recomb sums a level's recombination list -- the bound-free pairs of the ion below that lead to it -- 16 at a time. The
        # synthetic data let only an ion's lowest two levels recombine: what is pushed past 16 is the list each of them sums, not their number.
        assert int(d["nions"]) > 16
        starts, nlev = np.asarray(d["ion_uniquelevelindexstart"]), np.asarray(d["ion_nlevels"])
        tstart, ntargets = np.asarray(d["level_phixstargetstart"]), np.asarray(d["level_nphixstargets"])
        upper_level, nup = np.asarray(d["allphixstargets_levelindex"]), np.asarray(d["level_nuptrans"])
        lower = np.flatnonzero(np.asarray(d["ion_nlevels_ionising"]) > 0)
        assert len(lower) >= 12
        for ui in lower:
            first, last = starts[ui], starts[ui] + nlev[ui] - 1
            assert int(d["ion_maxrecombininglevel"][ui + 1]) >= 0
            assert np.count_nonzero(upper_level[tstart[first]:tstart[last] + ntargets[last]] == 0) > 16, ui
            assert np.count_nonzero(nup[first:last + 1] > 0) > 16, ui
    else:
        raise KeyError(name)


def table_range(options: str):
    """(MINTEMP, MAXTEMP) of the build's rate-coefficient tables (include/artis_options.h)"""
    t = abi.CI_PRESETS[options][2] if options in abi.CI_PRESETS else synth.OPTION_TABLES[options]
    return t[1], t[2]


EDGES = ("thick", "zero_massfrac", "one_ion", "te_lowest", "te_highest", "w_zero", "nne_tiny", "tr_far_below_te", "equilibrium", "renorm_zero")


def apply_edges(model, cs, options: str) -> dict:
    """Overwrites the first len(EDGES) cells of a synthetic cell state in place, one edge per cell, and leaves the rest alone. Returns
    edge name -> cell.
      thick            the cell is optically thick (W = 1): the expansion tables skip it
      zero_massfrac    element 0 has no mass: all its ions' populations are 0 (and the host's level populations of a no-LUT build)
      one_ion          the last element's first ion carries the whole element: the ground populations of its others are 0
      te_lowest / te_highest   T_e at the first / last temperature of the rate-coefficient tables
      w_zero           W = 0
      nne_tiny         nne = 1e-3
      tr_far_below_te  T_R = T_e / 20: stimulated corrections near 1
      equilibrium      T_R = T_e = T_J, W = 1: departure ratios near 1
      renorm_zero      corrphotoionrenorm 0 in the first ground continuum"""
    d, m = cs.d, model.d
    ncell, nions, nel = int(m["npts_nonempty"]), int(m["nions"]), int(m["nelements"])
    assert ncell > len(EDGES)
    cell = {name: k for k, name in enumerate(EDGES)}
    ground = d["ion_groundlevelpops"].reshape(ncell, nions)
    massfrac = d["elem_massfracs"].reshape(ncell, nel)
    hostpops = d["levelpops"].reshape(ncell, int(m["nlevels"])) if "levelpops" in d else None
    level_ion = np.repeat(np.arange(nions), np.asarray(m["ion_nlevels"]))

    def empty_ions(c, ions):
        ground[c, ions] = 0.0
        if hostpops is not None:
            hostpops[c, np.isin(level_ion, ions)] = 0.0

    c = cell["thick"]
    d["thick"][c], d["W"][c] = CELL_THICK, 1.0
    c = cell["zero_massfrac"]
    s0, n0 = int(m["elem_uniqueionindexstart"][0]), int(m["elem_nions"][0])
    massfrac[c, 0] = 0.0
    empty_ions(c, np.arange(s0, s0 + n0))
    c = cell["one_ion"]
    s1, n1 = int(m["elem_uniqueionindexstart"][nel - 1]), int(m["elem_nions"][nel - 1])
    assert n1 > 1
    total = float(ground[c, s1:s1 + n1].sum())
    empty_ions(c, np.arange(s1 + 1, s1 + n1))
    ground[c, s1] = total
    tmin, tmax = table_range(options)
    d["Te"][cell["te_lowest"]] = tmin
    d["Te"][cell["te_highest"]] = tmax
    d["W"][cell["w_zero"]] = 0.0
    d["nne"][cell["nne_tiny"]] = 1e-3
    c = cell["tr_far_below_te"]
    d["TR"][c] = d["Te"][c] / 20.0
    c = cell["equilibrium"]
    d["TR"][c] = d["TJ"][c] = d["Te"][c]
    d["W"][c] = 1.0
    assert int(m["nbfcontinua_ground"]) > 0
    d["corrphotoionrenorm"].reshape(ncell, int(m["nbfcontinua_ground"]))[cell["renorm_zero"], 0] = 0.0
    return cell
