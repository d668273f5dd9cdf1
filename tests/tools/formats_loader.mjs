// tests/tools/formats_loader.mjs — TEST INFRASTRUCTURE for tests/tools/make_formats_golden.py.  An ESM loader that lets the
// reference's PLY parsers import and run, unmodified and in place, under a Node that predates optional chaining:
//   resolve          the bare specifier 'three' resolves to oracle/three_min.mjs (what oracle/three_loader.mjs does)
//   transformSource  a rule on tokens, applied in memory to the reference's modules only: a statement
//                        return <expr> ?.<name>;      becomes      return ((<expr>) || {}).<name>;
//                    which means the same wherever <expr> is an object or undefined.
// usage: node --experimental-loader tests/tools/formats_loader.mjs tests/tools/formats_ref.mjs <reference/src> <dir>
import { pathToFileURL, fileURLToPath } from 'url';
import path from 'path';
const here = path.dirname(fileURLToPath(import.meta.url));
const shim = pathToFileURL(path.join(here, '..', '..', 'oracle', 'three_min.mjs')).href;
const own = pathToFileURL(path.join(here, '..', '..')).href;
export async function resolve(specifier, context, defaultResolve) {
  if (specifier === 'three') return { url: shim };
  return defaultResolve(specifier, context, defaultResolve);
}
const rule = /\breturn\s+([^;]*?)\s*\?\.\s*([A-Za-z_$][\w$]*)\s*;/gs;
export async function transformSource(source, context, defaultTransformSource) {
  if (context.url.startsWith(own + '/') || !context.url.startsWith('file:')) return defaultTransformSource(source, context, defaultTransformSource);
  const text = typeof source === 'string' ? source : Buffer.from(source).toString('utf8');
  return { source: text.replace(rule, 'return (($1) || {}).$2;') };
}
