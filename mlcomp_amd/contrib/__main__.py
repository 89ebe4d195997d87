"""``mlcomp-contrib``: k-fold split helpers writing ``fold.csv`` into the current folder
(`mlcomp/contrib/__main__.py:19-96`)."""
from __future__ import annotations

import os
import re
import uuid
from os.path import join

import click


def _grouper(regex):
    if not regex:
        return None
    pat = re.compile(regex)

    def get_group(x):
        m = pat.match(x)
        return m.group(1) if m else str(uuid.uuid4())
    return get_group


@click.group()
def main():
    pass


@main.command('split-pandas')
@click.argument('path')
@click.option('--n_splits', type=int, default=5)
def split_pandas(path, n_splits):
    import pandas as pd
    from mlcomp_amd.contrib.split import file_group_kfold
    df = pd.read_csv(path)
    folds = file_group_kfold(n_splits, image=list(df[df.columns[0]]))
    df['fold'] = folds['fold']   # index-aligned (the split shuffles rows)
    df.to_csv(join(os.getcwd(), 'fold.csv'), index=False)


@main.command('split-classify')
@click.argument('img_path')
@click.option('--n_splits', type=int, default=5)
@click.option('--group-regex')
def split_classify(img_path, n_splits, group_regex):
    from mlcomp_amd.contrib.split import file_group_kfold
    pairs = [(img, sub) for sub in sorted(os.listdir(img_path)) if os.path.isdir(join(img_path, sub))
             for img in sorted(os.listdir(join(img_path, sub)))]
    file_group_kfold(n_splits, join(os.getcwd(), 'fold.csv'), get_group=_grouper(group_regex),
                     image=[join(lab, img) for img, lab in pairs], label=[lab for _, lab in pairs])


@main.command('split-segment')
@click.argument('img_path')
@click.argument('mask_path')
@click.option('--n_splits', type=int, default=5)
@click.option('--group-regex')
def split_segment(img_path, mask_path, n_splits, group_regex):
    from mlcomp_amd.contrib.split import file_group_kfold
    file_group_kfold(n_splits, join(os.getcwd(), 'fold.csv'), get_group=_grouper(group_regex),
                     image=os.listdir(img_path), mask=os.listdir(mask_path), sort=True,
                     must_equal=['image', 'mask'])


@main.command('split-test-img')
@click.argument('img_path')
def split_test_img(img_path):
    import pandas as pd
    pd.DataFrame({'image': sorted(os.listdir(img_path)), 'fold': 0}).to_csv(
        join(os.getcwd(), 'fold_test.csv'), index=False)


@main.command('pack-records')
@click.argument('img_path')
@click.argument('out')
@click.option('--size', type=int, default=256, help='stored square size (shorter side resized, centre crop)')
@click.option('--fold-csv', default=None, help='fold.csv (image,label,fold): pack the rows of --fold only')
@click.option('--fold', type=int, default=None)
@click.option('--exclude-fold', is_flag=True, help='pack every fold except --fold (the training split)')
def pack_records(img_path, out, size, fold_csv, fold, exclude_fold):
    """Pack a class-per-folder image tree (or the rows of a fold.csv) into an .mlrec record
    file for the native input pipeline (mlcomp_amd.train.records)."""
    from mlcomp_amd.train.records import pack_images
    if fold_csv:
        import pandas as pd
        df = pd.read_csv(fold_csv)
        if fold is not None:
            df = df[(df['fold'] != fold) if exclude_fold else (df['fold'] == fold)]
        names = sorted(df['label'].astype(str).unique())
        paths = [join(img_path, p) for p in df['image']]
        labels = [names.index(str(v)) for v in df['label']]
    else:
        names = sorted(d for d in os.listdir(img_path) if os.path.isdir(join(img_path, d)))
        pairs = [(join(img_path, d, f), i) for i, d in enumerate(names) for f in sorted(os.listdir(join(img_path, d)))]
        paths, labels = [p for p, _ in pairs], [lab for _, lab in pairs]
    n = pack_images(paths, labels, out, size=size)
    with open(out + '.classes', 'w') as f:
        f.write('\n'.join(names) + '\n')
    click.echo(f'{n} images, {len(names)} classes -> {out}')


@main.command('pack-seg-records')
@click.argument('img_path')
@click.argument('mask_path')
@click.argument('out')
@click.option('--size', type=int, default=256, help='stored square size (shorter side resized, centre crop)')
@click.option('--kind', type=click.Choice(['planes', 'index']), default='planes',
              help='planes: non-zero mask bytes are foreground; index: the byte is the class id')
@click.option('--fold-csv', default=None, help='fold.csv (image,mask,fold): pack the rows of --fold only')
@click.option('--fold', type=int, default=None)
@click.option('--exclude-fold', is_flag=True, help='pack every fold except --fold (the training split)')
def pack_seg_records(img_path, mask_path, out, size, kind, fold_csv, fold, exclude_fold):
    """Pack an image folder and a mask folder (files paired by name, as split-segment pairs
    them) or the rows of a fold.csv into an image + mask .mlrec record file."""
    from mlcomp_amd.train.records import pack_seg_images
    if fold_csv:
        import pandas as pd
        df = pd.read_csv(fold_csv)
        if fold is not None:
            df = df[(df['fold'] != fold) if exclude_fold else (df['fold'] == fold)]
        images, masks = list(df['image']), list(df['mask'])
    else:
        by_stem = lambda n: os.path.splitext(n)[0]  # noqa: E731
        images, masks = sorted(os.listdir(img_path), key=by_stem), sorted(os.listdir(mask_path), key=by_stem)
    stem = lambda names: [os.path.splitext(n)[0] for n in names]  # noqa: E731
    if stem(images) != stem(masks):
        odd = sorted(set(stem(images)) ^ set(stem(masks)))
        raise click.ClickException(f'{img_path} and {mask_path} do not pair up by name'
                                   + (f': {", ".join(odd[:5])}' if odd else ' (order or duplicates)'))
    if not images:
        raise click.ClickException('no image / mask pairs')
    n = pack_seg_images([join(img_path, p) for p in images], [join(mask_path, p) for p in masks], out,
                        size=size, kind=kind)
    click.echo(f'{n} image / mask pairs ({kind}) -> {out}')


@main.command('pack-clip-records')
@click.option('--video-path', required=True, help='class/video/frames tree, or the root of the fold.csv video column')
@click.option('--out', required=True, help='the clip record file to write')
@click.option('--frames', type=int, required=True, help='frames stored per record')
@click.option('--size', type=int, default=128, help='stored square size (shorter side resized, centre crop)')
@click.option('--frame-step', type=int, default=1, help='take every n-th frame file of a folder')
@click.option('--pad-short', is_flag=True, help='repeat the last frame of a folder with too few frames')
@click.option('--fold-csv', default=None, help='fold.csv (video,label,fold): pack the rows of --fold only')
@click.option('--fold', type=int, default=None)
@click.option('--exclude-fold', is_flag=True, help='pack every fold except --fold (the training split)')
def pack_clip_records(video_path, out, frames, size, frame_step, pad_short, fold_csv, fold, exclude_fold):
    """Pack a class/video/frames tree of frame images (or the rows of a fold.csv, as
    VideoDataset reads them) into a clip record file for the native input pipeline
    (mlcomp_amd.train.records): per video the centred window of --frames frames."""
    from mlcomp_amd.train.records import pack_clip_frames
    if fold_csv:
        import pandas as pd
        df = pd.read_csv(fold_csv)
        if fold is not None:
            df = df[(df['fold'] != fold) if exclude_fold else (df['fold'] == fold)]
        names = sorted(df['label'].astype(str).unique())
        dirs = [join(video_path, p) for p in df['video']]
        labels = [names.index(str(v)) for v in df['label']]
    else:
        names = sorted(d for d in os.listdir(video_path) if os.path.isdir(join(video_path, d)))
        pairs = [(join(video_path, d, v), i) for i, d in enumerate(names)
                 for v in sorted(os.listdir(join(video_path, d))) if os.path.isdir(join(video_path, d, v))]
        dirs, labels = [p for p, _ in pairs], [lab for _, lab in pairs]
    if not dirs:
        raise click.ClickException('no video folders')
    try:
        n = pack_clip_frames(dirs, labels, out, frames=frames, size=size, frame_step=frame_step,
                             pad_short=pad_short)
    except ValueError as e:
        raise click.ClickException(str(e))
    with open(out + '.classes', 'w') as f:
        f.write('\n'.join(names) + '\n')
    click.echo(f'{n} clips of {frames} frames, {len(names)} classes -> {out}')


@main.command('pack-text-records')
@click.option('--csv', 'csv_path', required=True, help='the CSV with the text and label columns')
@click.option('--text-col', default='text', help='column of the (first) text')
@click.option('--text-b-col', default=None, help='column of the second text of a pair')
@click.option('--label-col', default='label')
@click.option('--vocab', required=True, help='the BERT vocab.txt the model was trained with')
@click.option('--out', required=True, help='the text record file to write')
@click.option('--max-len', type=int, default=128, help='longest record in tokens, [CLS] / [SEP] included')
@click.option('--cased', is_flag=True, help='keep case and accents (the cased models)')
@click.option('--fold-csv', default=None, help='fold.csv (a fold column, rows as in --csv): pack the rows of --fold only')
@click.option('--fold', type=int, default=None)
@click.option('--exclude-fold', is_flag=True, help='pack every fold except --fold (the training split)')
def pack_text_records(csv_path, text_col, text_b_col, label_col, vocab, out, max_len, cased, fold_csv, fold,
                      exclude_fold):
    """Tokenise a CSV with WordPiece over --vocab and pack it into a text record file for the
    native input pipeline (mlcomp_amd.train.records): [CLS] a [SEP] (b [SEP]) per row."""
    from mlcomp_amd.train.records import pack_text_csv
    try:
        n, names = pack_text_csv(csv_path, vocab, out, text_col=text_col, label_col=label_col,
                                 text_b_col=text_b_col, max_len=max_len, lower=not cased, fold_csv=fold_csv,
                                 fold=fold, exclude_fold=exclude_fold)
    except ValueError as e:
        raise click.ClickException(str(e))
    with open(out + '.classes', 'w') as f:
        f.write('\n'.join(names) + '\n')
    click.echo(f'{n} sequences, {len(names)} classes -> {out}')


if __name__ == '__main__':
    main()
