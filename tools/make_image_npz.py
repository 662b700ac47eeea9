#!/usr/bin/env python
"""Local image files -> the npz the training loops (``--data``) and the linear evaluation (``test_lineval.py --data``)
read: ``x_train`` / ``x_test`` uint8 [n, H, W, 3], ``y_train`` / ``y_test`` int64 [n].  Reads local files only.

    python tools/make_image_npz.py cifar  DIR  OUT.npz     # CIFAR python pickles: data_batch_* + test_batch (CIFAR-10)
                                                           #                       or train + test (CIFAR-100)
    python tools/make_image_npz.py folder ROOT OUT.npz [--size S]
                                                           # ROOT/{train,test}/<class>/*, read with PIL; classes are
                                                           # numbered in sorted order of the train split's directory names
"""
import argparse
import os
import pickle
import sys

import numpy as np

IMAGE_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')


def _unpickle(path):
    with open(path, 'rb') as f:
        d = pickle.load(f, encoding='latin1')
    data = np.asarray(d['data'], dtype=np.uint8)
    labels = d['labels'] if 'labels' in d else d['fine_labels']
    if data.ndim != 2 or data.shape[1] != 3072 or len(labels) != len(data):
        raise ValueError('%s: [n, 3072] uint8 rows with n labels expected, got %s and %d labels' % (path, data.shape, len(labels)))
    # a row is the image in CHW order (1024 red, 1024 green, 1024 blue values) -> [32, 32, 3]
    return data.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1), np.asarray(labels, dtype=np.int64)


def read_cifar(root):
    names = sorted(os.listdir(root))
    train = sorted((n for n in names if n.startswith('data_batch_')), key=lambda n: int(n.split('_')[-1])) or \
        [n for n in names if n == 'train']
    test = [n for n in names if n in ('test_batch', 'test')][:1]
    if not train or not test:
        raise ValueError('%s: neither data_batch_* + test_batch nor train + test found' % root)
    out = {}
    for split, files in (('train', train), ('test', test)):
        parts = [_unpickle(os.path.join(root, n)) for n in files]
        out['x_' + split] = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
        out['y_' + split] = np.concatenate([p[1] for p in parts])
    return out


def read_folder(root, size=None):
    from PIL import Image                                   # only this branch needs PIL
    classes = sorted(d for d in os.listdir(os.path.join(root, 'train')) if os.path.isdir(os.path.join(root, 'train', d)))
    if not classes:
        raise ValueError('%s/train holds no class directories' % root)
    out = {}
    for split in ('train', 'test'):
        xs, ys = [], []
        for label, cls in enumerate(classes):
            d = os.path.join(root, split, cls)
            if not os.path.isdir(d):
                continue
            for name in sorted(os.listdir(d)):
                if not name.lower().endswith(IMAGE_EXTENSIONS):
                    continue
                with Image.open(os.path.join(d, name)) as im:
                    im = im.convert('RGB')
                    if size is not None and im.size != (size, size):
                        im = im.resize((size, size), Image.BICUBIC)
                    xs.append(np.asarray(im, dtype=np.uint8))
                ys.append(label)
        if not xs:
            raise ValueError('%s/%s holds no images' % (root, split))
        shapes = set(x.shape for x in xs)
        if len(shapes) != 1:
            raise ValueError('%s/%s: images of different sizes %s (pass --size)' % (root, split, sorted(shapes)[:4]))
        out['x_' + split] = np.ascontiguousarray(np.stack(xs))
        out['y_' + split] = np.asarray(ys, dtype=np.int64)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('kind', choices=('cifar', 'folder'))
    ap.add_argument('source', help='directory of the pickles / root of the train and test trees')
    ap.add_argument('out', help='npz to write')
    ap.add_argument('--size', type=int, default=None, help='folder: resize every image to SIZE x SIZE (bicubic)')
    a = ap.parse_args(argv)
    data = read_cifar(a.source) if a.kind == 'cifar' else read_folder(a.source, a.size)
    np.savez(a.out, **data)
    print('%s: x_train %s, x_test %s, %d classes' % (a.out, data['x_train'].shape, data['x_test'].shape,
                                                    int(data['y_train'].max()) + 1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
