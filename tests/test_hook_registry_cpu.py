"""train_driver.HOOKS: the one list of monitoring hooks behind the three training scripts -- its order, what an untouched
command line parses to, every hook's flags through its check, and the refusal of a companion flag without its switch."""
import pytest
import torch

import hook_flags
from contrad_amd import contrast, knn, latent, prdc, spectrum, swd, train_driver

PARSERS = hook_flags.script_parsers()
KNN_ATTRIBUTES = {'knn_data': None, 'knn_k': 200, 'knn_temp': 0.1}


def test_the_registry_is_in_evaluation_order():
    """Grids, kNN, contrast, SWD, spectrum, PPL, PRDC: PRDC last, so that ``_best`` is decided before the checkpoint names."""
    assert train_driver.HOOKS == (train_driver.GRIDS, knn.HOOK, contrast.HOOK, swd.HOOK, spectrum.HOOK, latent.HOOK, prdc.HOOK)
    assert [hook.shown for hook in train_driver.HOOKS] == ['G', 'D', 'D', 'G', 'G', 'G', 'G']
    assert [hook.improved is not None for hook in train_driver.HOOKS] == [False] * 6 + [True]
    assert set(train_driver.HELP_ORDER) == set(train_driver.HOOKS[1:])              # every hook with flags of its own is added
    assert prdc.HOOK_DEFAULTS == prdc.HOOK.defaults and list(prdc.HOOK_DEFAULTS)[0] == 'prdc_data'


@pytest.mark.parametrize('script', list(PARSERS))
def test_a_minimal_command_line_leaves_only_the_knn_attributes_and_every_hook_off(script):
    was_initialised = torch.cuda.is_initialized()
    P = PARSERS[script](hook_flags.MINIMAL)
    names = [name for hook in train_driver.HOOKS for name in hook.defaults]
    assert len(names) == 3 + 3 + 2 + 2 + 4 + 11
    assert {name: getattr(P, name) for name in names if hasattr(P, name)} == KNN_ATTRIBUTES
    for hook in train_driver.HOOKS:
        H = hook.check(P)
        assert not hook.on(P) and vars(H) == hook.defaults, hook.switch
        assert not getattr(H, hook.switch, None)
    assert torch.cuda.is_initialized() == was_initialised


@pytest.mark.parametrize('script', list(PARSERS))
def test_every_hooks_flags_come_back_through_its_check(script):
    assert [hook.switch for hook in train_driver.HOOKS] == list(hook_flags.GIVEN)
    plain = vars(PARSERS[script](hook_flags.MINIMAL))
    for hook in train_driver.HOOKS:
        flags, want = hook_flags.GIVEN[hook.switch]
        P = PARSERS[script](hook_flags.MINIMAL + flags)
        assert set(want) == set(hook.defaults)                           # (the table gives every flag of the hook)
        assert hook.on(P) and vars(hook.check(P)) == want, hook.switch
        others = {k: v for k, v in vars(P).items() if k not in want and k != hook.switch}
        assert others == {k: v for k, v in plain.items() if k not in want and k != hook.switch}    # nothing else moves
        for other in train_driver.HOOKS:
            if other is not hook:
                assert not other.on(P) and vars(other.check(P)) == other.defaults


def test_a_stray_flag_is_refused_by_every_hook_but_knn():
    parse = PARSERS['train_gan']
    for hook in train_driver.HOOKS[1:]:
        P = parse(hook_flags.MINIMAL + hook_flags.STRAY[hook.switch])
        if hook is knn.HOOK:
            assert hook.check(P).knn_k == 20 and not hook.on(P)
            continue
        flag = hook_flags.STRAY[hook.switch][0]
        with pytest.raises(ValueError, match='^%s does nothing without --%s FILE' % (flag, hook.switch)):
            hook.check(P)
    # several: all of them are named, in the order of the flags
    with pytest.raises(ValueError, match='^--ppl_encoder_arch, --ppl_n, --ppl_space do nothing without --ppl_encoder FILE.pt$'):
        latent.check_hook_arguments(parse(hook_flags.MINIMAL + ['--ppl_space', 'z', '--ppl_n', '128', '--ppl_encoder_arch', 'sndcgan']))
    with pytest.raises(ValueError, match='^--prdc_k, --prdc_fd do nothing without --prdc_data FILE.npz$'):
        prdc.check_hook_arguments(parse(hook_flags.MINIMAL + ['--prdc_fd', '--prdc_k', '3']))


def test_the_modules_keep_their_entry_points_as_delegations():
    for module in (prdc, contrast, swd, spectrum, latent):
        assert module.add_hook_arguments == module.HOOK.add_arguments and module.check_hook_arguments == module.HOOK.check
    assert knn.add_hook_arguments == knn.HOOK.add_arguments and prdc.hook_options == prdc.HOOK.options
