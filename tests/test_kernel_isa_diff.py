"""CPU: scripts/kernel_isa_diff.py on two short made-up listings."""
import io
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import kernel_isa_diff as K  # noqa: E402

HEAD = "\t.text\n\t.globl\t%s\n%s:                             ; @%s\n; %%bb.0:\n"
TAIL = ("\ts_endpgm\n\t.amdhsa_kernel %s\n\t\t.amdhsa_private_segment_fixed_size %d\n\t\t.amdhsa_next_free_vgpr %d\n\t\t.amdhsa_accum_offset %d\n"
        "\t.end_amdhsa_kernel\n\t.text\n.Lfunc_end%d:\n\t.size\t%s, .Lfunc_end%d-%s\n\t.set %s.num_vgpr, %d\n; NumVgprs: %d\n")


def listing(path, kernels):
    """kernels: [(symbol, body text, private, vgpr, accum)] in file order"""
    with open(path, "w") as f:
        for n, (s, body, priv, vgpr, acc) in enumerate(kernels):
            f.write(HEAD % (s, s, s) + body + TAIL % (s, priv, vgpr, acc, n, s, n, s, s, vgpr, vgpr))
    return str(path)


A = "_Z5k_onePd"
B = "_Z8k_mc_camILb1EEvPd"
C = "_Z15k_mc_cam_chunksILb1EEvPd"
LOOP = "\tv_mov_b32_e32 v1, 0\n.LBB%d_1:                                ; =>This Inner Loop Header\n\tv_add_u32_e32 v1, 1, v1\n\ts_cbranch_vccnz .LBB%d_1\n"


def run(tmp_path, old, new, touched):
    out = io.StringIO()
    bad = K.compare(K.kernels(listing(tmp_path / "old.s", old)), K.kernels(listing(tmp_path / "new.s", new)), touched, out)
    return bad, out.getvalue()


def test_split_comments_and_labels(tmp_path):
    k = K.kernels(listing(tmp_path / "a.s", [(A, LOOP % (0, 0), 0, 4, 4), (B, "\tv_fma_f64 v[0:1], v[2:3], v[4:5], v[0:1] ; a comment\n", 0, 8, 8)]))
    assert list(k) == [A, B]
    assert k[A][:4] == ["v_mov_b32_e32 v1, 0", ".LBB_1:", "v_add_u32_e32 v1, 1, v1", "s_cbranch_vccnz .LBB_1"]
    assert k[B][0] == "v_fma_f64 v[0:1], v[2:3], v[4:5], v[0:1]" and not any(";" in x or ".size" in x for x in k[B])
    assert K.resources(k[B]) == {".amdhsa_next_free_vgpr": 8, ".amdhsa_accum_offset": 8, ".amdhsa_private_segment_fixed_size": 0}
    assert [K.source_name(s) for s in (A, B, C)] == ["k_one", "k_mc_cam", "k_mc_cam_chunks"]


def test_same_kernels_in_another_order_are_identical(tmp_path):
    """a function's number in its local labels and the comments are not part of a body"""
    old = [(A, LOOP % (0, 0), 0, 4, 4), (B, "\tv_mul_f64 v[0:1], v[2:3], v[4:5]\n", 0, 8, 8)]
    new = [(B, "\tv_mul_f64 v[0:1], v[2:3], v[4:5] ; other words\n", 0, 8, 8), (A, LOOP % (1, 1), 0, 4, 4)]
    bad, text = run(tmp_path, old, new, set())
    assert bad == 0 and "symbol sets equal" in text and "bodies: 2 identical, 0 differ" in text


def test_histogram_counts_arithmetic_not_encodings(tmp_path):
    body = ("\tv_fmac_f32_e32 v0, v1, v2\n\tv_fma_f32 v3, v1, v2, v3\n\tv_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[0:1]\n\tv_mul_f64 v[0:1], v[2:3], v[4:5]\n"
            "\tv_subrev_f32_e32 v0, v1, v2\n\tv_div_scale_f64 v[0:1], vcc, v[2:3], v[2:3], v[4:5]\n\tv_rcp_f64_e32 v[0:1], v[2:3]\n\tv_sqrt_f32_e32 v0, v1\n"
            "\tv_add_u32_e32 v0, v1, v2\n\tv_mul_lo_u32 v0, v1, v2\n\tv_cvt_f32_f64_e32 v0, v[2:3]\n\tv_max_f32_e32 v0, v1, v2\n\tglobal_load_dwordx2 v[0:1], v2, s[0:1]\n")
    h = K.fp_histogram(K.kernels(listing(tmp_path / "a.s", [(A, body, 0, 8, 8)]))[A])
    assert h == {"v_fma_f32": 2, "v_pk_fma_f32": 1, "v_mul_f64": 1, "v_sub_f32": 1, "v_div_scale_f64": 1, "v_rcp_f64": 1, "v_sqrt_f32": 1}


def test_report_and_verdict(tmp_path):
    fused = "\tv_fma_f32 v0, v1, v2, v0\n"
    moved = "\tv_mov_b32_e32 v9, v8\n\tv_fmac_f32_e32 v0, v1, v2\n"
    unfused = "\tv_mul_f32_e32 v3, v1, v2\n\tv_add_f32_e32 v0, v0, v3\n"
    old = [(A, LOOP % (0, 0), 0, 4, 4), (B, fused, 0, 8, 8), (C, fused, 0, 8, 8)]
    # a rescheduled body with the same arithmetic: reported, accepted when its kernel is listed (k_mc_cam does not list k_mc_cam_chunks)
    bad, text = run(tmp_path, old, [old[0], (B, moved, 0, 12, 12), old[2]], {"k_mc_cam"})
    assert bad == 0 and "DIFFERS    " + B in text and "fp opcodes equal" in text and "bodies: 2 identical, 1 differ" in text
    assert ".amdhsa_next_free_vgpr                   8    12" in text
    bad, text = run(tmp_path, old, [old[0], old[1], (C, moved, 0, 8, 8)], {"k_mc_cam"})
    assert bad == 1 and "NOT LISTED" in text
    # a changed contraction, a new private segment, a missing symbol: each a finding
    bad, text = run(tmp_path, old, [old[0], (B, unfused, 0, 8, 8), old[2]], {"k_mc_cam"})
    assert bad == 1 and "fp opcodes DIFFER" in text and "v_fma_f32" in text and "<--" in text
    assert run(tmp_path, old, [old[0], (B, moved, 16, 8, 8), old[2]], {"k_mc_cam"})[0] == 1
    bad, text = run(tmp_path, old, old[:2], {"k_mc_cam"})
    assert bad == 1 and "symbol sets DIFFER" in text and "only in old: " + C in text
    # without a list the script only reports
    assert run(tmp_path, old, [old[0], (B, unfused, 0, 8, 8), old[2]], None)[0] == 0
    assert K.main([str(tmp_path / "old.s"), str(tmp_path / "old.s"), "--touched", "k_one"]) == 0
