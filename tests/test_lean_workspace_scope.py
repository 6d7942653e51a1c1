"""The lean workspace's switch (ops.lean_workspace_scope, ops.lean_workspace, SCNERF_LEAN_WORKSPACE): "off", "render" (the
default: the render step alone, as before the scope existed) or "all" (the NeRF++ node and the network query node as
well).  No GPU needed."""
import pytest

from scnerf_amd import ops


@pytest.fixture
def scope():
    before = ops.lean_workspace_scope()
    yield ops.lean_workspace_scope
    ops.lean_workspace_scope(before)


def test_every_environment_value_accepted_before_keeps_its_meaning():
    # (before the scope: unset -> on, "" and "0" -> off, anything else -> on -- for the render step, the only taker)
    assert ops._lean_scope_from_env(None) == "render"
    assert ops._lean_scope_from_env("") == "off" and ops._lean_scope_from_env("0") == "off"
    for value in ("1", "on", "yes", "true", "render", "2"):
        assert ops._lean_scope_from_env(value) == "render", value
    assert ops._lean_scope_from_env("all") == "all"


def test_the_boolean_switch_is_the_render_steps_view_of_the_scope(scope):
    assert scope("all") == "all" and ops.lean_workspace() is True
    assert ops.lean_workspace(True) is True and scope() == "render"
    assert ops.lean_workspace(False) is False and scope() == "off"
    assert scope("render") == "render" and ops.lean_workspace() is True
    assert scope("off") == "off" and ops.lean_workspace() is False
    with pytest.raises(ValueError):
        scope("everything")
    assert scope() == "off"


def test_the_lean_checks_accept_both_point_dimensions_and_keep_every_refusal():
    class Packs:
        fast = False
    one_product = Packs()
    one_product.fast = True
    save = maxima = object()
    for pd in (3, 4):
        ops._check_lean(True, pd, save, maxima, Packs())
        for args in ((pd, None, maxima, Packs()), (pd, save, None, Packs()), (pd, save, maxima, one_product)):
            with pytest.raises(ValueError):
                ops._check_lean(True, *args)
    with pytest.raises(ValueError):
        ops._check_lean(True, 5, save, maxima, Packs())
    ops._check_lean(False, 5, None, None, one_product)
