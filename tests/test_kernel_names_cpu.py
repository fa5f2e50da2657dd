"""tests/kernel_names.py: the mangled keys of kernel_resources.json split into
(kernel name, template arguments) by walking the name's components, on
hand-written keys.  Runs without a GPU and without a build."""
import pytest

import kernel_names as K

ANON = "_ZN3apg12_GLOBAL__N_1"


def test_plain_kernel():
    assert K.split_key(ANON + "22lstm_gate_wgrad_kernelENS0_6GwArgsE") == \
        ("lstm_gate_wgrad_kernel", "")
    # ... and the kernel whose name begins with it is another kernel
    assert K.split_key(ANON + "29lstm_gate_wgrad_reduce_kernelENS0_12GwReduceArgsE") == \
        ("lstm_gate_wgrad_reduce_kernel", "")


def test_template_arguments():
    assert K.split_key(ANON + "21cart_mpc_solve_kernelILi5EEEvNS0_16CartMpcSolveArgsE") == \
        ("cart_mpc_solve_kernel", "ILi5E")
    assert K.split_key(ANON + "27cart_mpc_closed_loop_kernelILi10ELb1EEEvNS0_15CartMpcLoopArgsE") \
        == ("cart_mpc_closed_loop_kernel", "ILi10ELb1E")
    assert K.split_key(ANON + "11some_kernelILb0ELb1EEEvPf") == ("some_kernel", "ILb0ELb1E")
    # a negative literal, a type argument, a named type argument
    assert K.split_key(ANON + "11some_kernelILin3EfNS0_3FooEEEvPf") == \
        ("some_kernel", "ILin3EfNS0_3FooE")
    with pytest.raises(ValueError):                # a list that never closes
        K.split_key(ANON + "11some_kernelILi5")


def test_outside_the_anonymous_namespace():
    assert K.split_key("_ZN3apg13to_soa_kernelEPKfPfii") == ("to_soa_kernel", "")
    assert K.split_key("_ZN3apgL18learnt_pack_kernelE17ApgLearntResidualPf") == \
        ("learnt_pack_kernel", "")
    assert K.split_key("_ZL19copy_unroll4_kernelILb1EEvPKDv4_fPS0_x") == \
        ("copy_unroll4_kernel", "ILb1E")
    assert K.split_key("_ZL16copy_flat_kernelPKDv4_fPS_x") == ("copy_flat_kernel", "")


def test_not_a_mangled_name():
    for key in ("cart_mpc_solve_kernel", "_ZN3apg99shortE", "_ZN3apg", "_ZN3apg5shortv"):
        with pytest.raises(ValueError):
            K.split_key(key)


def _res(*keys):
    return {k: {"key": k} for k in keys}


def test_instances_match_the_whole_name():
    """A kernel is no instance of a kernel whose name is a part of its own."""
    solve = [ANON + f"21cart_mpc_solve_kernelILi{h}EEEvNS0_16CartMpcSolveArgsE" for h in (5, 10)]
    learnt = [ANON + f"28cart_mpc_learnt_solve_kernelILi{h}EEEvNS0_22CartLearntMpcSolveArgsE"
              for h in (5, 10)]
    # (a name CONTAINING the other one, which a substring search would count)
    inner = ANON + "27my_cart_mpc_solve_kernel_v2ILi5EEEvPf"
    res = _res(*solve, *learnt, inner)
    got = K.instances(res, "cart_mpc_solve_kernel")
    assert sorted(got) == ["ILi10E", "ILi5E"]
    assert got["ILi5E"] == {"key": solve[0]} and got["ILi10E"] == {"key": solve[1]}
    assert sorted(K.instances(res, "cart_mpc_learnt_solve_kernel")) == ["ILi10E", "ILi5E"]
    assert K.instances(res, "cart_mpc_learnt_solve_kernel")["ILi5E"] == {"key": learnt[0]}
    assert K.instances(res, "solve_kernel") == {}


def test_quad_closed_loops_are_two_kernels():
    ana = [ANON + f"27quad_mpc_closed_loop_kernelILb{p}EEEvNS0_11MpcLoopArgsE" for p in (0, 1)]
    learnt = [ANON + f"34quad_learnt_mpc_closed_loop_kernelILb{p}EEEvNS0_11MpcLoopArgsEPKf"
              for p in (0, 1)]
    res = _res(*ana, *learnt)
    got = K.instances(res, "quad_mpc_closed_loop_kernel")
    assert {k: v["key"] for k, v in got.items()} == {"ILb0E": ana[0], "ILb1E": ana[1]}
    got = K.instances(res, "quad_learnt_mpc_closed_loop_kernel")
    assert {k: v["key"] for k, v in got.items()} == {"ILb0E": learnt[0], "ILb1E": learnt[1]}
    assert K.instances(res, "mpc_closed_loop_kernel") == {}
