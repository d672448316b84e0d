"""The trust-region core of k_lm_solve and k_map_solve (lmono_amd/csrc/trust_region.hpp), host build of the same header, driven by
scripted sums through the branches no scan pair and no map scene reaches.  Every expected value follows from the rules of the loop:

The pose is the identity, the gradient has a translation component g alone, H = I unless said otherwise.  Then scale = 1 / (1 + sqrt(1)) =
0.5, the scaled system is 0.25 I with the gradient 0.5 g, the diagonal taken for the damping is 0.25, and at the start radius of 1e4 the
step is -0.5 g / 0.250025 in scaled and about -g in pose units, with a model change of about g^2 / 2.

1   g = 0: begin() says there is nothing to do; no iteration is counted.
2   H with a zero diagonal and ones elsewhere: the damped diagonal is min_diag / radius = 1e-10, the first pivot 1e-5, the second
    1e-10 - 1e10 < 0: the factorisation fails whatever the radius is.  max_iter 4: four invalid steps, each halves the radius
    (1e4 / 16 = 625), then the iterations are used up.
3   the same with max_iter 8: the fifth invalid step ends the solve before it halves the radius again (iter 5, radius 625).
4   max_iter 64, g = 1e26, every candidate costs 2 against 1: every step is rejected.  The k-th rejection divides the radius by 2^k
    (decrease_factor doubles), so after k of them it is 1e4 / 2^(k (k + 1) / 2), exactly, these being powers of two; the diagonal is
    taken once and reused from the second damping on (0.25 throughout).  2^105 = 4.06e31 and 2^120 = 1.33e36: the radius is 2.5e-28 after
    14 rejections and 7.5e-33 <= min_radius = 1e-32 after 15, where judge() ends the solve.  The smallest radius a step is made with is
    2.5e-28: damping 1e27, step 0.5e26 / 1e27 = 0.05, far above parameter_tol, so no other exit interferes.
5   max_iter 1, g = 1, cost 0.5 -> 0: propose() says "cost only" (1); the step is accepted (relative decrease 0.5 / 0.49999.. = 1.0),
    x becomes the candidate, and since nothing after the last accepted step is used, take() is not called and the radius stays 1e4.
6   the same with max_iter 4 and a candidate whose gradient is zero: accepted, take() once, radius 1e4 / (1 / 3) = 3e4 (rho = 1 gives
    1 - (2 rho - 1)^3 = 0, raised to 1 / 3), then the gradient test ends the solve.  6b: a candidate gradient of 1e-3 instead: the loop goes on.
7   g = 1e-9, cost 1 -> 0.5: the step is 1e-9 <= parameter_tol (|x| + parameter_tol) = 1e-8: exit, although the cost would have been accepted.
8   g = 1, cost 1 -> 1 - 5e-7: the change is within function_tol = 1e-6 of the cost: exit; without that rule the step would be rejected
    (relative decrease 5e-7 / 0.5 < 1e-3) and judge() would say go on with radius 5e3.
2 to 4 run with both damping forms, diag / radius (k_map_solve) and diag * (1 / radius) (k_lm_solve)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REJECTED = "rejects=15,iter=15,full_eval=1,radius_rule=1,reuse_rule=1,takes=0,x_kept=1,below_min=1,prev_above_min=1"
EXPECTED = " | ".join([
    "1:begin=0,iter=0",
    "2<0>:ctl=2,iter=4,invalid=4,radius=625",
    "2<1>:ctl=2,iter=4,invalid=4,radius=625",
    "3<0>:ctl=2,iter=5,invalid=5,radius=625",
    "3<1>:ctl=2,iter=5,invalid=5,radius=625",
    "4<0>:" + REJECTED,
    "4<1>:" + REJECTED,
    "5:ctl=1,judge=0,takes=0,x=cand,iter=1,radius=10000",
    "6:ctl=0,judge=0,takes=1,x=cand,iter=1,radius=30000",
    "6b:ctl=0,judge=1,takes=1,x=cand,iter=1,radius=30000",
    "7:ctl=0,judge=0,takes=0,x=start,iter=1,radius=10000",
    "8:ctl=0,judge=0,takes=0,x=start,iter=1,radius=10000",
])


def test_trust_region_branches_no_scene_reaches(tmp_path):
    exe = str(tmp_path / "trust_region_check")
    subprocess.check_call(["g++", "-O2", os.path.join(ROOT, "tests", "trust_region_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.strip() == EXPECTED
