"""Markdown table of the step / adjoint kernels' resources, read from redmax_amd/kernel_fingerprint.json (what __graft_entry__.build()
wrote for the library it linked): the one source of the register / scratch figures quoted in DESIGN.md.   python tools/kernel_table.py"""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (  # (name fragment, what it runs)
    ("k_step_bdf1_pair32", "configs[1] headline: full 32-link chain, BDF1, two points per front"),
    ("k_step_bdf1<32, false, false, true, 0>", "the one-point kernel of the same chain (RMX_PAIRC=0; bit-identity reference)"),
    ("k_step_bdf1<32, false, false, true, 16>", "the same chain, two wavefronts per rollout (RMX_PAIRC=0, 128..512 rollouts)"),
    ("k_step_bdf1<64, false, false, false, 18>", "configs[2]: full 64-node tree, two wavefronts per rollout (<= 512 rollouts), no energy record"),
    ("k_step_bdf1<64, false, false, false, 16>", "the same with the per-step energy record"),
    ("k_step_bdf1<64, false, false, false, 19>", "configs[2] at > 512 rollouts: constants in global memory, four wavefronts per CU"),
    ("k_ground32", "configs[4]: 32-link chain on frictional ground, BDF2, rollouts + cooperative groups in one launch"),
    ("k_step_pair<false>", "the same as separate launches: rollouts"),
    ("k_step_pair<true>", "... and cooperative groups"),
    ("k_adjoint_fwd<16, 1, true, true>", "configs[3]: adjoint BDF1 forward sweep, full 16-link chain, second wavefront for M, D (<= 512 rollouts)"),
    ("k_adjoint_fwd<16, 1, false, true>", "the same, one wavefront per rollout (larger batches)"),
    ("k_adjoint_bwd<16, 1, true>", "configs[3]: backward sweep"),
    ("k_adjoint_fwd<64, 1, false, false>", "adjoint forward, 33..64 nodes"),
    ("k_adjoint_fwd<16, 13, true, true>", "rmx_adjoint_track (per-step controls + tracking objective), BDF1: forward sweep, full 16-link chain, second wavefront"),
    ("k_adjoint_bwd<16, 13, true>", "rmx_adjoint_track: backward sweep, full 16-link chain"),
    ("k_adjoint_fwd<64, 13, false, false>", "rmx_adjoint_track: forward sweep, 33..64 nodes"),
    ("k_adjoint_fwd<16, 21, true, true>", "rmx_rollout_tape (taped forward sweep, BDF1): full 16-link chain, second wavefront"),
    ("k_adjoint_bwd<16, 21, true>", "rmx_rollout_vjp (cotangents in, du, dq0, dqd0 out): full 16-link chain"),
    ("k_adjoint_fwd<64, 21, false, false>", "rmx_rollout_tape: 33..64 nodes"),
    ("k_adjoint_bwd<32, 21, false>", "rmx_rollout_vjp: 17..32 nodes"),
    ("k_adjoint_fwd<16, 22, false, true>", "rmx_rollout_tape_bdf2 (taped forward sweep, BDF2, SDIRK2a stage on the tape): full 16-link chain"),
    ("k_rollout_bwd_bdf2<16, true>", "rmx_rollout_vjp on a BDF2 tape: full 16-link chain"),
    ("k_adjoint_fwd<64, 22, false, false>", "rmx_rollout_tape_bdf2: 33..64 nodes"),
    ("k_rollout_bwd_bdf2<64, false>", "rmx_rollout_vjp on a BDF2 tape: 33..64 nodes"),
    ("k_adjoint_fwd<16, 85, false, false>", "rmx_rollout_tape_feedback (taped forward sweep under per-step affine state feedback, BDF1): 9..16 nodes"),
    ("k_adjoint_fwd<32, 85, false, false>", "rmx_rollout_tape_feedback, BDF1: 17..32 nodes"),
    ("k_adjoint_fwd<64, 85, false, false>", "rmx_rollout_tape_feedback, BDF1: 33..64 nodes"),
    ("k_adjoint_fwd<32, 86, false, false>", "rmx_rollout_tape_feedback, BDF2: 17..32 nodes"),
    ("k_adjoint_fwd<32, 21, false, false>", "rmx_rollout_tape, 17..32 nodes: the open-loop sibling of the feedback kernel"),
    ("k_rollout_bwd_fb<16, 1>", "rmx_rollout_vjp_feedback (closed-loop backward sweep: duff, dK, dxref, dq0, dqd0), BDF1 tape: 9..16 nodes"),
    ("k_rollout_bwd_fb<32, 1>", "rmx_rollout_vjp_feedback, BDF1 tape: 17..32 nodes"),
    ("k_rollout_bwd_fb<64, 1>", "rmx_rollout_vjp_feedback, BDF1 tape: 33..64 nodes"),
    ("k_rollout_bwd_fb<32, 2>", "rmx_rollout_vjp_feedback, BDF2 tape: 17..32 nodes"),
    ("k_rollout_bwd_fb<64, 2>", "rmx_rollout_vjp_feedback, BDF2 tape: 33..64 nodes"),
    ("k_rollout_bwd_bdf2<32, false>", "rmx_rollout_vjp on a BDF2 tape, 17..32 nodes: the open-loop sibling of `k_rollout_bwd_fb<32, 2>`"),
    ("k_rollout_linearize<4>", "rmx_rollout_linearize (XA, XB, XU of every slot of a tape; one wavefront per rollout and slot): <= 4 nodes"),
    ("k_rollout_linearize<8>", "rmx_rollout_linearize: 5..8 nodes"),
    ("k_rollout_linearize<16>", "rmx_rollout_linearize: 9..16 nodes"),
    ("k_rollout_linearize<32>", "rmx_rollout_linearize: 17..32 nodes, the four blocks in one pass"),
    ("k_rollout_linearize<64>", "rmx_rollout_linearize: 33..64 nodes, half a right-hand block per pass"),
    ("k_rollout_jvp<4>", "rmx_rollout_jvp (forward sweep over a tape; one wavefront per rollout and chunk of 8 tangent directions): <= 4 nodes"),
    ("k_rollout_jvp<8>", "rmx_rollout_jvp: 5..8 nodes"),
    ("k_rollout_jvp<16>", "rmx_rollout_jvp: 9..16 nodes"),
    ("k_rollout_jvp<32>", "rmx_rollout_jvp: 17..32 nodes"),
    ("k_rollout_jvp<64>", "rmx_rollout_jvp: 33..64 nodes, H, 8 columns and the carried tangents in registers"),
    ("k_rollout_lqr<8, false>", "rmx_rollout_lqr (Riccati sweep of iLQR over a BDF1 tape; one workgroup of 256 threads per rollout, Vxx in LDS): 5..8 nodes"),
    ("k_rollout_lqr<16, false>", "rmx_rollout_lqr: 9..16 nodes"),
    ("k_rollout_lqr<32, false>", "rmx_rollout_lqr: 17..32 nodes (145 664 bytes of LDS)"),
    ("k_rollout_lqr<8, true>", "rmx_rollout_lqr_box (the same sweep with the box QP of control-limited DDP in the place of the solve): 5..8 nodes"),
    ("k_rollout_lqr<16, true>", "rmx_rollout_lqr_box: 9..16 nodes"),
    ("k_rollout_lqr<32, true>", "rmx_rollout_lqr_box: 17..32 nodes (147 712 bytes of LDS)"),
    ("k_rollout_search<4>", "rmx_rollout_search (the line search of iLQR: every trial pass and the nominal pass of the closed loop, the cost inside the launch; one wavefront per rollout): <= 4 nodes"),
    ("k_rollout_search<8>", "rmx_rollout_search: 5..8 nodes"),
    ("k_rollout_search<16>", "rmx_rollout_search: 9..16 nodes"),
    ("k_rollout_search<32>", "rmx_rollout_search: 17..32 nodes, M and D on the matrix cores"),
    ("k_rollout_param_grad<4>", "rmx_rollout_vjp_params (the contraction over the slots of a tape; one wavefront per rollout): <= 4 nodes"),
    ("k_rollout_param_grad<8>", "rmx_rollout_vjp_params: 5..8 nodes"),
    ("k_rollout_param_grad<16>", "rmx_rollout_vjp_params: 9..16 nodes"),
    ("k_rollout_param_grad<32>", "rmx_rollout_vjp_params: 17..32 nodes"),
    ("k_rollout_param_grad<64>", "rmx_rollout_vjp_params: 33..64 nodes"),
    ("k_adjoint_bwd<16, 53, true>", "rmx_rollout_vjp_params: the BDF1 backward sweep that also stores z per slot, full 16-link chain"),
    ("k_adjoint_bwd<32, 53, false>", "the same, 17..32 nodes"),
    ("k_adjoint_bwd<64, 53, false>", "the same, 33..64 nodes"),
    ("k_rollout_bwd_bdf2_zs<16, true>", "rmx_rollout_vjp_params on a BDF2 tape: backward sweep with z per slot, full 16-link chain"),
    ("k_rollout_bwd_bdf2_zs<64, false>", "the same, 33..64 nodes"),
    ("k_step_bdf1<32, true, false, false, 0>", "generic contact / Euler-chart kernel, <= 32 nodes, BDF1"),
    ("k_step_bdf2<32, true, false, false, 0>", "generic contact / Euler-chart kernel, <= 32 nodes, BDF2"),
    ("k_big_step", "trees of 65..256 nodes (one workgroup per rollout)"),
    ("k_step_pf<32, 1>", "body-to-body forces (rmx_pf.h), <= 32 nodes, BDF1"),
    ("k_step_pf<32, 2>", "body-to-body forces, <= 32 nodes, BDF2"),
    ("k_step_pf<64, 1>", "body-to-body forces, 33..64 nodes, BDF1"),
    ("k_step_pf<64, 2>", "body-to-body forces, 33..64 nodes, BDF2"),
    ("k_tape_pf<4, 1, false>", "taped rollout with body-to-body forces (rmx_tape_pf.h), <= 4 nodes, BDF1"),
    ("k_tape_pf<8, 1, false>", "taped rollout with body-to-body forces, 5..8 nodes, BDF1"),
    ("k_tape_pf<16, 1, false>", "taped rollout with body-to-body forces, 9..16 nodes, BDF1"),
    ("k_tape_pf<32, 1, false>", "taped rollout with body-to-body forces, 17..32 nodes, BDF1"),
    ("k_tape_pf<32, 2, true>", "taped rollout with body-to-body forces, 17..32 nodes, BDF2, feedback stage"),
    ("k_tape_pf<64, 1, false>", "taped rollout with body-to-body forces, 33..64 nodes, BDF1"),
    ("k_tape_pf<64, 2, false>", "taped rollout with body-to-body forces, 33..64 nodes, BDF2"),
    ("k_tape_pf<64, 2, true>", "taped rollout with body-to-body forces, 33..64 nodes, BDF2, feedback stage"),
    ("k_rollout_force_grad<4>", "rmx_rollout_vjp_forces (the contraction for the force constants over the slots of a tape, rmx_force_params.h; one wavefront per rollout): <= 4 nodes"),
    ("k_rollout_force_grad<8>", "rmx_rollout_vjp_forces: 5..8 nodes"),
    ("k_rollout_force_grad<16>", "rmx_rollout_vjp_forces: 9..16 nodes"),
    ("k_rollout_force_grad<32>", "rmx_rollout_vjp_forces: 17..32 nodes"),
    ("k_rollout_force_grad<64>", "rmx_rollout_vjp_forces: 33..64 nodes"),
)


def main():
    fp = json.load(open(os.path.join(ROOT, "redmax_amd", "kernel_fingerprint.json")))
    print("| kernel | runs | VGPR+AGPR | scratch B/lane | SGPR spills | instructions |")
    print("|---|---|---|---|---|---|")
    for frag, what in ROWS:
        hit = [v for v in fp.values() if frag in v["name"]]
        for v in hit[:2 if "k_big_step" in frag else 1]:
            nm = v["name"].replace("void ", "").split("(")[0].replace("(anonymous namespace)::", "")
            print("| `%s` | %s | %d | %d | %d | %d |" % (nm, what, v["vgpr"], v["scratch_bytes"], v["sgpr_spills"], v["instructions"]))


main()
