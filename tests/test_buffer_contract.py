"""Every workspace-taking entry point of include/uglad_hip.h held to its buffers at run time (buffer_contract.py: the harness and what it
asserts; buffer_contract_cases.py: the cases).  The harness's self-tests run on CPU tensors with no library, so that it provably can fail;
the emulated subset runs the real kernels on the SIMT emulator; the GPU cases are one pytest id each, so that a failure names its route."""
import pytest
import torch

import buffer_contract as bc
import buffer_contract_cases as cases_


# ---------------------------------------------------------------------------------------------------------------- the harness can fail
class _Fake:
    """A 'call' on CPU tensors: 16 floats of output from 16 floats of input through a workspace of 8, with one defect switched on."""
    id, device, exempt = "fake", "cpu", None

    def __init__(self, defect=None):
        self.defect = defect

    def inputs(self):
        return {"x": torch.arange(16, dtype=torch.float32)}

    def call(self, inp):
        x = inp["x"]
        wsp = self.workspace()
        out = torch.empty(16, dtype=torch.float32, device="cpu")
        wsp[:4] = x[:4]  # the call defines words 0 .. 3 of its workspace and reads them back
        out[:] = x * 2.0 + wsp[:4].sum()
        byte = lambda t, at: torch.as_strided(t.view(torch.uint8), (1,), (1,), t.storage_offset() * t.element_size() + at)  # noqa: E731
        guarded = out._base is not None  # (the plain run has nothing around its buffers to write into)
        if self.defect == "left" and guarded:
            byte(out, -100)[0] = 1  # one byte, 100 before the output
        elif self.defect == "right" and guarded:
            byte(out, 64 + 7)[0] = 1  # one byte, 7 past its end
        elif self.defect == "stale":
            out[3] = wsp[6]  # a workspace word the call never wrote
        elif self.defect == "input":
            x[2] = -1.0
        elif self.defect == "rc":
            return {"out": out, "rc": -2}
        return {"out": out}

    def workspace(self):
        return torch.empty(8, dtype=torch.float32, device="cpu")


@pytest.fixture(autouse=True)
def _the_fake_workspace_is_scratch(monkeypatch):
    monkeypatch.setitem(bc.SCRATCH_SITES, ("test_buffer_contract.py", "workspace", None), "the fake call's workspace")


class _Unwritten(_Fake):
    def call(self, inp):
        x = inp["x"]
        out = torch.empty(16, dtype=torch.float32, device="cpu")
        out[:5] = x[:5] * 2.0
        out[6:] = x[6:] * 2.0  # element 5 is never written
        return {"out": out}


def test_a_clean_fake_call_passes():
    res = bc.run_case(_Fake())
    assert res.ok and not res.problems
    (okey, (onb, olo, ohi, oscr)), = [(k, v) for k, v in res.touched.items() if k.endswith(":out")]
    assert (onb, olo, oscr) == (64, 0, False) and ohi >= 60  # (under fill 0x00, x[0] * 2 + 6 = 6.0 has nonzero bytes: the union covers the start)
    (wkey, (wnb, wlo, whi, wscr)), = [(k, v) for k, v in res.touched.items() if not k.endswith(":out")]
    assert (wnb, wlo, whi, wscr) == (32, 0, 15, True)  # words 0 .. 3 only


def test_a_byte_in_the_left_guard_is_reported_with_its_offset():
    with pytest.raises(AssertionError, match=r"confinement \[fill 0x00\]: buffer \d+ out .*left guard changed at bytes -100 \.\. -100 \(1 bytes\)"):
        bc.run_case(_Fake("left"))
    res = bc.run_case(_Fake("left"), raise_on_failure=False)
    assert not res.confinement and res.independence and res.inputs_untouched and res.rc == 0


def test_a_byte_in_the_right_guard_is_reported_with_its_offset():
    with pytest.raises(AssertionError, match=r"confinement \[fill 0xFF\]: buffer \d+ out .*right guard changed at bytes 71 \.\. 71 \(1 bytes\)"):
        bc.run_case(_Fake("right"))
    res = bc.run_case(_Fake("right"), raise_on_failure=False)
    assert not res.confinement and res.independence and res.inputs_untouched and res.rc == 0


def test_an_unwritten_output_element_is_reported():
    with pytest.raises(AssertionError, match=r"independence \[fill 0x.. vs plain\]: output \d+:out .*differs at bytes 2[0-3] \.\. 2[0-3] \("):
        bc.run_case(_Unwritten())
    res = bc.run_case(_Unwritten(), raise_on_failure=False)
    assert res.confinement and not res.independence and res.inputs_untouched and res.rc == 0
    assert res.touched[[k for k in res.touched if k.endswith(":out")][0]][1:3] == (0, 63)  # (the extent says nothing of the hole: the comparison does)


def test_a_stale_workspace_word_copied_into_the_output_is_reported():
    with pytest.raises(AssertionError, match=r"independence \[fill 0x.. vs plain\]: output \d+:out .*differs at bytes 1[2-5] \.\. 1[2-5] \("):
        bc.run_case(_Fake("stale"))
    res = bc.run_case(_Fake("stale"), raise_on_failure=False)
    assert res.confinement and not res.independence and res.inputs_untouched and res.rc == 0


def test_a_modified_input_is_reported():
    with pytest.raises(AssertionError, match=r"inputs \[plain\]: x changed at bytes 10 \.\. 11 "):
        bc.run_case(_Fake("input"))
    res = bc.run_case(_Fake("input"), raise_on_failure=False)
    assert res.confinement and not res.inputs_untouched and res.rc == 0


def test_a_nonzero_return_code_is_reported():
    res = bc.run_case(_Fake("rc"), raise_on_failure=False)
    assert res.confinement and res.independence and res.inputs_untouched and res.rc == -2 and not res.ok


def test_buffers_of_another_device_pass_through_unguarded():
    real = torch.empty
    with bc.guarded_buffers("cpu", 0x7F) as gb:
        meta = torch.empty(5, 3, device="meta")
        mine = torch.empty(5, 3, dtype=torch.float64)
        like = torch.empty_like(meta)
    assert torch.empty is real
    assert meta.device.type == "meta" and like.device.type == "meta"
    assert [b.shape for b in gb.buffers] == [(5, 3)] and gb.buffers[0].view is mine
    assert mine.dtype == torch.float64 and mine.is_contiguous() and mine.data_ptr() % 64 == 0
    assert bool((mine == torch.tensor([0x7F7F7F7F7F7F7F7F]).view(torch.float64)).all())  # 1.38e306, finite
    assert gb.buffers[0].raw.numel() == 5 * 3 * 8 + 2 * bc.GUARD_BYTES


def test_zero_size_requests_and_every_way_to_give_a_shape():
    with bc.guarded_buffers("cpu", 0xFF) as gb:
        a = torch.empty(0, dtype=torch.float32)
        b = torch.empty((2, 0, 3), dtype=torch.int32)
        c = torch.empty(torch.Size([4]), dtype=torch.int32)
        d = torch.empty_like(torch.zeros(2, 2, dtype=torch.float64))
        e = torch.empty((), dtype=torch.float32)
    assert a.shape == (0,) and b.shape == (2, 0, 3) and c.shape == (4,) and d.shape == (2, 2) and e.shape == ()
    assert bool((c == -1).all()) and bool(torch.isnan(d).all()) and bool(torch.isnan(e))
    reps = gb.check()
    assert len(reps) == 5 and all(r.confined and r.touched is None for r in reps)
    c[1] = 7
    assert gb.check()[2].touched == (4, 7)  # word 1


def test_the_patch_is_gone_after_the_block_raises():
    real, real_like = torch.empty, torch.empty_like
    with pytest.raises(RuntimeError, match="inside"):
        with bc.guarded_buffers("cpu", 0x00):
            assert torch.empty is not real
            raise RuntimeError("inside")
    assert torch.empty is real and torch.empty_like is real_like

    class Raises(_Fake):
        def call(self, inp):
            raise KeyError("the call itself fails")

    with pytest.raises(KeyError):
        bc.run_case(Raises())
    assert torch.empty is real and torch.empty_like is real_like


def test_guard_bytes_keep_the_alignment():
    with pytest.raises(ValueError):
        bc.guarded_buffers("cpu", 0, guard_bytes=1000)
    assert bc.GUARD_BYTES % 512 == 0 and bc.GUARD_BYTES == 2 * 64 * 64 * 8


def test_every_exemption_quotes_the_header():
    import os

    header = " ".join(open(os.path.join(os.path.dirname(__file__), "..", "include", "uglad_hip.h")).read().replace(" * ", " ").split())
    assert sorted(bc.EXEMPTIONS) == ["graph_wide.edges", "matrix_iteration.beta"]  # nothing is added to it
    for ex in bc.EXEMPTIONS.values():
        quote = ex.header.split('"')[1]
        assert " ".join(quote.split()) in header, quote


def test_every_scratch_site_exists_in_the_wrappers():
    """A buffer is scratch by where it is allocated; a site that is renamed away would make its buffer an output (and the case fail), one
    that never existed would be a dead entry."""
    import glob
    import os
    import re

    root = os.path.join(os.path.dirname(__file__), "..", "uglad_amd")
    for (fname, func, name), why in bc.SCRATCH_SITES.items():
        if fname == "test_buffer_contract.py":
            continue
        (path,) = glob.glob(os.path.join(root, "**", fname), recursive=True)
        body = re.search(rf"\n    def {func}\(.*?(?=\n    def |\n    @|\nclass |\Z)", open(path).read(), re.S)
        assert body, (fname, func)
        assert re.search(rf"\b{name} = .*torch\.empty\(" if name else r"return torch\.empty\(", body.group(0)), (fname, func, name, why)


# ---------------------------------------------------------------------------------------------------------------- the cases
EMULATED = cases_.cases("cpu", emulated=True)
GPU = cases_.cases("cuda")


@pytest.mark.parametrize("case", EMULATED, ids=[c.id for c in EMULATED])
def test_emulated(emul, case):
    bc.run_case(case)


@pytest.fixture(scope="module")
def lib():
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU, ids=[c.id for c in GPU])
def test_gpu(lib, case):
    bc.run_case(case)


@pytest.mark.gpu
def test_the_kendall_case_is_dealt_over_several_chunks(lib):
    assert lib.rank_pair_chunks(*cases_.KENDALL_CHUNKED) > 1
