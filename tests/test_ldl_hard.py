"""The L D L^T inverse and log-determinant (csrc/ldl_wide.h + the two Newton steps of launch_ns_inverse) against numpy fp64 on hard matrices, and
its exact properties.  GPU tests (marked gpu) and their CPU twins on the SIMT emulator run the same checks on the inputs of ldl_cases.hard_matrix,
through lib.loss_fwd with S = 0 (the loss is -logdet) and lib.init_theta, under both kernel forms (UGLAD_LDL_LAUNCHES = 0 / 1).

Against fp64, from the input alone (ldl_cases.reference64; u = 2^-24, X64 = A^-1, L, d the fp64 unpivoted factors):
  1. inverse      ||X - X64||_F / ||X64||_F <= C_INV u || |X64| |A| |X64| ||_F / ||X64||_F
  2. logdet       |logdet - slogdet| <= u (sum_ij |X64|_ij (|L| |d| |L|^T)_ij + sqrt(D) max_k |sum_{i<=k} ln |d_i||) + ulp32(logdet) / 2, and that bound
                  is itself below ldl_cases.LOGDET_CAP on the kinds of ldl_cases.LOGDET_CAPPED (the rest have element growth: the bound is printed)
  3. residual     ||A X - I||_F / sqrt(D) next to torch32's: printed, not asserted (1 bounds it)
Exact, no tolerance:
  4. scaling      X(2^k A) 2^k has the bits of X(A), k = -20, 7, 20; the log-determinant moves by D k ln 2 within the summation term of 2
  5. symmetry     X = X^T bit for bit
  6. isolation    every matrix of a mixed batch has the bits and the NaN pattern it has alone, under both forms alike
  7. sign rule    k = 0 .. 5 negative pivots in different 32-blocks: the loss is NaN exactly for odd k (torch.logdet in fp64), else within 2
No figure here comes from a run of the code under test; every test prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

import ldl_cases as lc

# Bound 1's constant: twice the largest ratio (error / unit bound) torch.linalg.inv reaches IN FP32 ON THE CPU on the inputs of this module -- the
# reference's own arithmetic; the two is for the other accumulation order of the MFMA products, a margin over the reference, not over the
# device.  Measured over every (kind, D) bound 1 is asserted on (scripts/ldl_probe.py --hard prints the column): torch32 peaks on "graded", and by how
# much depends on the CPU's BLAS blocking: 1.63 / 1.60 / 1.90 of the unit bound at D = 129 / 161 / 577 on one machine, 1.64 / 1.98 / 1.93 on
# another (profiles/ldl_hard_errors.txt); the next kind is "sign4" at 0.54, every other one stays below 0.25.  2 x 1.98, rounded up.
C_INV = 4.0
FORMS = ("0", "1")
SCALE_KINDS = ("spd_1e2", "flip40_1e2")  # 4: one spd, one indefinite input
SCALE_K = (-20, 7, 20)

_runs = {}  # what a device returned for an input, shared by the tests of a session and left unchanged


def run_batch(lib, dev, entry, kinds, D, form, k=0):
    """(X, loss) of ONE call on the matrices [(kind, seed), ...] scaled by 2^k."""
    key = (dev, entry, tuple(kinds), D, form, k)
    if key not in _runs:
        A = np.stack([lc.hard_matrix(kind, D, seed) for kind, seed in kinds]) * np.float32(2.0 ** k)
        _runs[key] = lc.run_on(lib, dev, entry, A, form)
    return _runs[key]


def run_one(lib, dev, kind, D, form, seed=0, k=0):
    X, loss = run_batch(lib, dev, lc.entry_of(kind), ((kind, seed),), D, form, k)
    return X[0], None if loss is None else loss[0]


def check_inverse(tag, X, ref):
    """1 and 5 for one finite inverse."""
    ex, bound = lc.inverse_error(X, ref), C_INV * ref["inv_unit"]
    print(f"{tag}: inverse error {ex:.3e}, {ex / ref['inv_unit']:.3f} of the unit bound {ref['inv_unit']:.3e} (allowed: {C_INV})")
    assert X.tobytes() == X.T.tobytes(), f"{tag}: X is not X^T bit for bit"
    assert ex <= bound, f"{tag}: inverse error {ex:.3e} > {bound:.3e}"


def check_logdet(tag, loss, ref, capped):
    """2 for one finite log-determinant (loss = -logdet)."""
    el = abs(-float(loss) - ref["logdet"])
    print(f"{tag}: logdet error {el:.3e}, bound {ref['ld_bound']:.3e} (growth {ref['growth']:.1e}, summation term {ref['sum_term']:.1e})")
    if capped:
        assert ref["ld_bound"] < lc.LOGDET_CAP, f"{tag}: the bound says nothing: {ref['ld_bound']:.3e}"
    assert el <= ref["ld_bound"], f"{tag}: logdet error {el:.3e} > {ref['ld_bound']:.3e}"


def check_family(lib, dev, kind, D):
    """1, 2, 3, 5 for one kind under both forms, and that the forms agree."""
    a, ref = lc.hard_matrix(kind, D, 0), lc.hard_reference(kind, D, 0)
    A = lc.inverted(kind, a)
    t_inv, _ = lc.torch32(lc.shifted32(a) if lc.entry_of(kind) == "init" else a)
    outs = {}
    for form in FORMS:
        tag = f"{kind} D={D} {lc.form_id(form)}"
        X, loss = outs[form] = run_one(lib, dev, kind, D, form)
        print(f"{tag}: ||A X - I||_F / sqrt(D) {lc.residual(A, X):.3e} (torch32 {lc.residual(A, t_inv):.3e}, its inverse error "
              f"{lc.inverse_error(t_inv, ref) / ref['inv_unit']:.3f} of the unit bound)")
        check_inverse(tag, X, ref)
        if lc.entry_of(kind) == "init":  # Theta_0 comes without a log-determinant: the same pivots through the loss, from the matrix kLdlInit forms
            a_t = lc.shifted32(a)
            ref_t = lc.reference64(a_t.astype(np.float64), spd=False)
            loss = lc.run_on(lib, dev, "loss", a_t[None], form)[1][0]
            if np.isnan(ref_t["logdet"]):
                assert np.isnan(loss), tag
            else:
                check_logdet(tag + " (through the loss)", loss, ref_t, lc.logdet_capped(kind, D))
        else:
            check_logdet(tag, loss, ref, lc.logdet_capped(kind, D))
    assert lc.same_bits(outs["0"][0], outs["1"][0]), f"{kind} D={D}: the two forms differ"


def check_scaling(lib, dev, kind, D, forms=FORMS):
    """4 for one input."""
    a = lc.hard_matrix(kind, D, 0).astype(np.float64)
    d = lc.pivots64(a, spd=D > lc.SPD_SHORTCUT_BEYOND and kind in lc.SPD_KINDS)
    for form in forms:
        X0, loss0 = run_one(lib, dev, kind, D, form)
        assert np.isfinite(X0).all() and np.isfinite(loss0), (kind, D, form)
        for k in SCALE_K:
            Xk, lossk = run_one(lib, dev, kind, D, form, k=k)
            moved = (-float(lossk)) - (-float(loss0)) - D * k * np.log(2.0)
            bound = (lc.sum_term(d) + lc.sum_term(d * 2.0 ** k) + 0.5 * float(np.spacing(np.float32(abs(lossk))))
                     + 0.5 * float(np.spacing(np.float32(abs(loss0)))))
            print(f"{kind} D={D} {lc.form_id(form)} k={k}: logdet {-float(lossk):.6g}, off D k ln 2 by {moved:.3e}, bound {bound:.3e}")
            assert (Xk * np.float32(2.0 ** k)).tobytes() == X0.tobytes(), f"{kind} D={D} k={k}: X(2^k A) 2^k is not X(A)"
            assert abs(moved) <= bound, f"{kind} D={D} k={k}: logdet moved by D k ln 2 {moved:+.3e}, bound {bound:.3e}"


def check_isolation(lib, dev, D, forms):
    """6 at one size.  forms: the forms to run (None = the default among them); each matrix runs alone under the first, and every form's batch has
    the bits of the first form's."""
    first = run_batch(lib, dev, "loss", lc.BATCH_KINDS, D, forms[0])
    for form in forms:
        X, loss = run_batch(lib, dev, "loss", lc.BATCH_KINDS, D, form)
        print(f"D={D} {lc.form_id(form)}: loss of the batch {loss}")
        assert lc.same_bits(X, first[0]) and lc.same_bits(loss, first[1]), f"D={D}: {lc.form_id(form)} differs from {lc.form_id(forms[0])}"
    X, loss = first
    for m, (kind, seed) in enumerate(lc.BATCH_KINDS):
        Xm, lm = run_one(lib, dev, kind, D, forms[0], seed=seed)
        assert lc.same_bits(X[m], Xm), f"D={D}: matrix {m} ({kind}) of the batch is not what it is alone"
        assert lc.same_bits(loss[m], lm), f"D={D}: loss {m} ({kind}) of the batch is not what it is alone"
        if kind == "pivot0":
            assert np.isnan(X[m]).all() and np.isnan(loss[m]), f"D={D}: a zero first pivot is NaN throughout"
        elif kind == "neg3":
            assert np.isnan(loss[m]), f"D={D}: three negative eigenvalues, det < 0: NaN (torch.logdet's rule)"
            check_inverse(f"batch[{m}] {kind} D={D}", X[m], lc.hard_reference(kind, D, seed))
        else:
            assert np.isfinite(X[m]).all() and np.isfinite(loss[m]), f"D={D}: matrix {m} ({kind})"


def check_sign_rule(lib, dev, D):
    """7 at one size."""
    for k in range(len(lc.SIGN_AT) + 1):
        kind = f"sign{k}"
        ref = lc.hard_reference(kind, D, 0)
        want_nan = bool(torch.isnan(torch.logdet(torch.from_numpy(lc.hard_matrix(kind, D, 0).astype(np.float64)))))
        blocks = sorted(set(np.flatnonzero(ref["d"] < 0) // 32))
        print(f"{kind} D={D}: negative pivots in the 32-blocks {blocks}")
        assert want_nan == (k % 2 == 1) and len(blocks) == k  # (the input is what it is meant to be)
        for form in FORMS:
            X, loss = run_one(lib, dev, kind, D, form)
            tag = f"{kind} D={D} {lc.form_id(form)}"
            assert np.isnan(loss) == want_nan, f"{tag}: loss {loss}, torch.logdet in fp64 is {'NaN' if want_nan else 'finite'}"
            check_inverse(tag, X, ref)
            if not want_nan:
                check_logdet(tag, loss, ref, capped=False)


# ---- CPU: the SIMT emulator.  Its eigensolver ends at D = 160, so 161 is on this path (nt = 6, ragged last tile); 200 = the size of the older cases
EMUL_D = 161


@pytest.mark.parametrize("kind", lc.FAMILIES)
def test_emulated_inverse_and_logdet_within_the_fp64_bounds(emul, kind):
    check_family(emul, "cpu", kind, EMUL_D)


@pytest.mark.parametrize("kind", SCALE_KINDS)
def test_emulated_scaling_by_powers_of_two_is_exact(emul, kind):
    check_scaling(emul, "cpu", kind, EMUL_D)


@pytest.mark.parametrize("D", [EMUL_D, 200])
def test_emulated_batch_isolation(emul, D):
    check_isolation(emul, "cpu", D, FORMS)


@pytest.mark.parametrize("D", [EMUL_D, 200])
def test_emulated_sign_rule_across_blocks(emul, D):
    check_sign_rule(emul, "cpu", D)


# ---- GPU
@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from uglad_amd import _lib

    return _lib.get_lib()


# 129: nt = 5, ragged tile, first size on this path; 577: nt = 19 > 16 waves, the tile loops of the one-workgroup walk and the capped element grids wrap
@pytest.mark.gpu
@pytest.mark.parametrize("D", [129, 577])
@pytest.mark.parametrize("kind", lc.FAMILIES)
def test_inverse_and_logdet_within_the_fp64_bounds(lib, kind, D):
    check_family(lib, "cuda", kind, D)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SCALE_KINDS)
def test_scaling_by_powers_of_two_is_exact(lib, kind):
    check_scaling(lib, "cuda", kind, 129)


# the default form changes at nt = 9: one workgroup per matrix at 129 and 256, launches at 257 and 288
@pytest.mark.gpu
@pytest.mark.parametrize("D", [129, 257, 288])
def test_batch_isolation(lib, D):
    check_isolation(lib, "cuda", D, FORMS + (None,))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [129, 288])
def test_sign_rule_across_blocks(lib, D):
    check_sign_rule(lib, "cuda", D)


@pytest.mark.gpu
def test_two_matrices_in_the_2048_wide_layout_through_the_loss(lib):
    """D = 1025: FD = 2048, nt = 33, with a batch: the slab stride of the wide layout, which Theta_0 alone reaches elsewhere."""
    D, kinds = 1025, (("flip40_1e2", 0), ("spd_1e3", 1))  # one indefinite with element growth (2 uncapped), one spd (capped)
    outs = {form: run_batch(lib, "cuda", "loss", kinds, D, form) for form in FORMS}
    for form, (X, loss) in outs.items():
        for m, (kind, seed) in enumerate(kinds):
            tag, ref = f"batch[{m}] {kind} D={D} {lc.form_id(form)}", lc.hard_reference(kind, D, seed)
            check_inverse(tag, X[m], ref)
            check_logdet(tag, loss[m], ref, lc.logdet_capped(kind, D))
    assert lc.same_bits(outs["0"][0], outs["1"][0]) and lc.same_bits(outs["0"][1], outs["1"][1])


@pytest.mark.gpu
def test_the_largest_size(lib):
    """D = 2048: 1, 2 and 5 on the spd input, 4 on it and on the indefinite one.  2^(+-20 D) overflows every
    float format: k = +-20 also shows that the determinant is never formed as a product."""
    D = 2048
    ref = lc.hard_reference(SCALE_KINDS[0], D, 0)
    for form in FORMS:
        X, loss = run_one(lib, "cuda", SCALE_KINDS[0], D, form)
        check_inverse(f"{SCALE_KINDS[0]} D={D} {lc.form_id(form)}", X, ref)
        check_logdet(f"{SCALE_KINDS[0]} D={D} {lc.form_id(form)}", loss, ref, capped=True)
    for kind in SCALE_KINDS:
        check_scaling(lib, "cuda", kind, D)
        for form in FORMS:
            X = run_one(lib, "cuda", kind, D, form)[0]
            assert X.tobytes() == X.T.tobytes(), f"{kind} D={D} {lc.form_id(form)}: X is not X^T bit for bit"
