"""One valid command line per monitoring hook of the training scripts, keyed by the hook's switch: (the flags, what the
hook's check must hand back).  Shared by the tests that walk train_driver.HOOKS."""
MINIMAL = ['cfg.gin', 'sndcgan']

GIVEN = {
    'monitor': (['--monitor'], {}),
    'knn_data': (['--knn_data', 'l.npz', '--knn_k', '20', '--knn_temp', '0.5'], dict(knn_data='l.npz', knn_k=20, knn_temp=0.5)),
    'contrast_data': (['--contrast_data', 'x.npz', '--contrast_n', '500', '--contrast_t', '3'],
                      dict(contrast_data='x.npz', contrast_n=500, contrast_t=3.0)),
    'swd_data': (['--swd_data', 'x.npz', '--swd_n', '64'], dict(swd_data='x.npz', swd_n=64)),
    'spectrum_data': (['--spectrum_data', 'x.npz', '--spectrum_n', '9'], dict(spectrum_data='x.npz', spectrum_n=9)),
    'ppl_encoder': (['--ppl_encoder', 'e.pt', '--ppl_encoder_arch', 'snresnet18', '--ppl_n', '128', '--ppl_space', 'z'],
                    dict(ppl_encoder='e.pt', ppl_encoder_arch='snresnet18', ppl_n=128, ppl_space='z')),
    'prdc_data': (['--prdc_data', 'x.npz', '--prdc_encoder', 'e.pt', '--prdc_encoder_arch', 'snresnet18', '--prdc_k', '3', '--prdc_n', '192',
                   '--prdc_best', 'kid', '--prdc_kid', '--prdc_kid_kernel', 'rq', '--prdc_auth', '--prdc_fd', '--prdc_fd_iter', '30'],
                  dict(prdc_data='x.npz', prdc_encoder='e.pt', prdc_encoder_arch='snresnet18', prdc_k=3, prdc_n=192, prdc_best='kid',
                       prdc_kid=True, prdc_kid_kernel='rq', prdc_auth=True, prdc_fd=True, prdc_fd_iter=30)),
}

# one companion flag without its switch: refused by every hook but kNN, whose flags have ordinary defaults
STRAY = {'knn_data': ['--knn_k', '20'], 'contrast_data': ['--contrast_n', '500'], 'swd_data': ['--swd_n', '64'],
         'spectrum_data': ['--spectrum_n', '9'], 'ppl_encoder': ['--ppl_n', '128'], 'prdc_data': ['--prdc_k', '3']}


def script_parsers():
    """``parse_args`` of the three training scripts."""
    from contrad_amd import train_gan, train_stylegan2
    return {'train_gan': train_gan.parse_args, 'train_stylegan2': train_stylegan2.parse_args,
            'train_stylegan2_contraD': lambda argv: train_stylegan2.parse_args(argv, contrad_script=True)}
